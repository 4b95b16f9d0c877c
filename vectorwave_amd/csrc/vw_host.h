// vw_host.h -- private to the C-ABI host layer (vw_ctx.cpp, vw_exec.cpp, vw_api_*.cpp): the handle types, the
// thread's error state, launch timing, the staged call (Staging), workspace growth, the argument checks, the
// call-record builders and the two executors.  One way to do each: an entry point checks its arguments, builds
// its FwdCall / InvCall once, opens a Staging, runs the device function and returns finish() ("Where kernel selection lives").
#pragma once
#include "../../include/vectorwave_amd.h"
#include "vw_launch.h"
#include "vw_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

namespace vw {

// ------------------------------------------------------------------------------------------------
// Errors (thread-local, like the reference's exceptions are per call site); defined once, in vw_ctx.cpp
struct ErrState {
  std::string msg;
  int64_t index = -1;
  int64_t signal_base = 0;  // run_sharded: global row of this block's first signal
};
ErrState& err_state();
vw_status fail(vw_status code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
vw_status ok();

#define VW_HIP(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) return fail(VW_ERR_DEVICE, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

#define VW_TRY(expr)                      \
  do {                                    \
    vw_status s_ = (expr);                \
    if (s_ != VW_OK) return s_;           \
  } while (0)

struct TimedLaunch {
  std::string family;
  hipEvent_t start, stop;
  bool graph_owned = false;  // recorded inside a captured graph: its events live as long as the graph
};

// A forward recorded during the current capture that the NEXT call may turn into a round trip (try_pair_fuse):
// its kernel node, and the call as it was launched.  No pointer of the caller's that may die is kept: the taps
// are in `args`.
struct PairPending {
  bool valid = false;
  hipGraphNode_t node = nullptr;
  FwdCall<double> call;
  FwdPlan<double> plan;
  FwdArgs<double> args;
};

}  // namespace vw

struct vw_graph;

struct vw_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool capturing = false;      // between vw_capture_begin / vw_capture_end
  unsigned ws_gen = 0;         // bumped when ws / ws2 move: graphs recorded before are stale
  vw::Tuning tune;
  int cus = 256;               // compute units of the device (small-batch policies)
  std::recursive_mutex mu;
  void* ws = nullptr;          // tiled-path ping-pong buffers
  size_t ws_bytes = 0;
  void* ws2 = nullptr;         // denoise coefficients / thresholds
  size_t ws2_bytes = 0;
  unsigned long long* bad = nullptr;   // device word for the fused non-finite check
  bool timing = false;
  std::vector<vw::TimedLaunch> pending;
  std::vector<vw::TimedLaunch> captured;   // timed launches recorded during the current capture
  std::vector<hipEvent_t> event_pool;
  std::map<std::string, std::pair<double, int64_t>> totals;
  std::set<vw_graph*> graphs;          // live graphs recorded on this context (invalidated at destroy)
  std::vector<std::pair<void*, size_t>> stage;  // host-memory staging pool (Staging), kept across calls
  void* med = nullptr;         // vw_median_f64 deviations of long rows (not ws: growing ws invalidates graphs)
  size_t med_bytes = 0;
  int* nf = nullptr;           // VW_FLAG_REF_NONFINITE row flags [nf_rows], zero between calls (vw_ref.hip)
  int64_t nf_rows = 0;
  vw::PairPending pair;        // VW_PAIR_FUSE: the forward the next call may fuse with (capture only)
  int fused_pairs = 0;         // round trips recorded by the current capture
  void* cwt_dev = nullptr;     // vw_cwt_*: the scale descriptors and tap tables of the last call, on the device
  size_t cwt_dev_bytes = 0;
  std::vector<unsigned char> cwt_img;  // ... and the host image they were copied from (a call with the same one uploads nothing)
  void* icwt_dev = nullptr;    // vw_icwt_*: the same for the inverse, in a slot of its own (alternating calls keep both images)
  size_t icwt_dev_bytes = 0;
  std::vector<unsigned char> icwt_img;
};

struct vw_graph {
  vw_ctx* ctx = nullptr;          // nullptr once the context is destroyed (the graph is then dead)
  int device = 0;
  unsigned ws_gen = 0;
  std::vector<vw::TimedLaunch> timed;  // event-record nodes (timing enabled at capture)
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int fused_pairs = 0;             // forward -> inverse pairs recorded as one k_roundtrip node
};

struct vw_stream {
  vw_ctx* ctx = nullptr;
  std::vector<double> lo, hi;
  int L = 0;
  int boundary = 0;
  int levels = 0;
  int64_t last_batch = -1;
  bool hist_init = false;
  std::vector<double*> hist;        // device [B][hist_len_j]
  std::vector<double*> snap;        // VW_FLAG_REF_NONFINITE: the histories a block read (same shapes)
  std::vector<int> hist_len;
};

namespace vw {

// Brackets a kernel launch with HIP events on the context stream when timing is enabled.  While
// capturing, the events become event-record nodes of the graph (hipEventRecordExternal), owned by
// the graph: every replay re-records them, so the launch is timed inside the replayed graph.
struct LaunchTimer {
  vw_ctx* c;
  TimedLaunch tl;
  bool on;
  LaunchTimer(vw_ctx* ctx, const char* family);
  ~LaunchTimer();
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Grows the context buffer *buf (of *have bytes) to hold `bytes`, allocating at least `min_bytes`.  A buffer that
// moves may have been used on streams the context was bound to before, and recorded graphs hold its address: the
// device is drained and ws_gen bumped (vw_graph_launch then refuses those graphs).  Refused during a capture;
// `what` names the buffer in that message.
vw_status grow_buffer(vw_ctx* c, void** buf, size_t* have, size_t bytes, size_t min_bytes, const char* what);
inline vw_status ensure_ws(vw_ctx* c, size_t bytes) {
  return grow_buffer(c, &c->ws, &c->ws_bytes, bytes, (size_t)1 << 20, "workspace");
}
inline vw_status ensure_ws2(vw_ctx* c, size_t bytes) {
  return grow_buffer(c, &c->ws2, &c->ws2_bytes, bytes, 0, "workspace");
}

// ------------------------------------------------------------------------------------------------
// The one path of a call into the device: takes the context's mutex and makes its device current, then
//   Staging s(c, flags);  VW_TRY(s.open());  s.in / s.out on the call's pointers;  run with s.flags();  return s.finish();
// With VW_FLAG_HOST_MEMORY (the JNI / FFM path) in / out replace a host pointer by a device buffer carved from the
// context's staging pool (blocks kept across calls, never hipMalloc / hipFree per call: a JNI caller's per-batch
// loop pays only the copies and the kernels), inputs copied in at once, outputs copied back by finish().  A call
// carves from offset 0 of the pool; the stream is synchronized before the call returns, so the next call may reuse
// the same bytes.  Without the flag in / out leave the pointers alone: no HIP call, no allocation.
struct Staging {
  Staging(vw_ctx* ctx, unsigned flags);
  ~Staging();  // a staged call: the stream is drained (also on an error path) and the pool trimmed to its largest block
  // Calls that synchronize cannot be recorded into a graph: refused before the first copy, the capture stays valid.
  vw_status open() const;
  bool host() const { return fl & VW_FLAG_HOST_MEMORY; }
  // the flags of the device function: finish() owns the synchronize, the pointers are the device's
  unsigned flags() const { return fl & ~(unsigned)(VW_FLAG_SYNC | VW_FLAG_HOST_MEMORY); }

  // Inputs.  A null pointer stays null.  in_planes: `planes` blocks of `count` elements, the host blocks
  // `host_stride` elements apart (a row block of a [planes][B][N] host array), packed on the device.
  template <typename T>
  vw_status in_planes(const T** p, size_t planes, size_t count, size_t host_stride) {
    if (!host() || !*p) return VW_OK;
    void* d = nullptr;
    VW_TRY(copy_in(*p, planes, count * sizeof(T), host_stride * sizeof(T), &d));
    *p = static_cast<const T*>(d);
    return VW_OK;
  }
  template <typename T>
  vw_status in(const T** p, size_t count) { return in_planes(p, 1, count, count); }
  // rows [B][ld] of N elements: the last row's padding need not exist
  template <typename T>
  vw_status in_rows(const T** p, int64_t B, int64_t N, int64_t ld) { return in(p, (size_t)(B - 1) * ld + N); }
  // staged on device-pointer calls too (host data of the call's own making)
  template <typename T>
  vw_status upload(const T* host, size_t count, const T** dev) {
    void* d = nullptr;
    VW_TRY(copy_in(host, 1, count * sizeof(T), count * sizeof(T), &d));
    *dev = static_cast<const T*>(d);
    return VW_OK;
  }

  // Outputs: *p becomes a device buffer that finish() copies to the host array it was.
  template <typename T>
  vw_status out_planes(T** p, size_t planes, size_t count, size_t host_stride) {
    if (!host() || !*p) return VW_OK;
    void* d = nullptr;
    VW_TRY(reserve_out(*p, planes, count * sizeof(T), host_stride * sizeof(T), &d));
    *p = static_cast<T*>(d);
    return VW_OK;
  }
  template <typename T>
  vw_status out(T** p, size_t count) { return out_planes(p, 1, count, count); }
  // updated in place: copied in, and back
  template <typename T>
  vw_status inout(T** p, size_t count) {
    T* const h = *p;
    VW_TRY(out(p, count));
    return host() ? copy(*p, h, 1, count * sizeof(T), 0, hipMemcpyHostToDevice) : VW_OK;
  }

  // The registered copy-outs, the synchronize of a staged or VW_FLAG_SYNC call, ok().
  vw_status finish();

 private:
  struct Out { void* host; const void* dev; size_t planes, bytes, stride; };
  vw_ctx* const c;
  const unsigned fl;
  std::unique_lock<std::recursive_mutex> lock;
  size_t used_block = 0, used_off = 0;
  bool carved = false, synced = false;
  Out outs[4];
  int nouts = 0;
  vw_status carve(size_t bytes, void** out);
  vw_status copy(void* dst, const void* src, size_t planes, size_t bytes, size_t host_stride, hipMemcpyKind kind);
  vw_status copy_in(const void* host, size_t planes, size_t bytes, size_t host_stride, void** dev);
  vw_status reserve_out(void* host, size_t planes, size_t bytes, size_t host_stride, void** dev);
};

// ------------------------------------------------------------------------------------------------
// Common argument checks (MultiLevelMODWTTransform.decompose :209-239, BatchMODWT.validateAoS :201-212)
inline vw_status check_common(vw_ctx* c, const void* a, const void* b, const double* lo, const double* hi,
                              int64_t B, int64_t N, int L, int boundary) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  if (!a || !b || !lo || !hi) return fail(VW_ERR_NULL, "null array argument");
  if (B <= 0) return fail(VW_ERR_EMPTY, "batch must be non-empty (B=%lld)", (long long)B);
  if (N <= 0) return fail(VW_ERR_EMPTY, "Signal cannot be empty");
  if (N > (1LL << 30)) return fail(VW_ERR_ARG, "signal length %lld too large", (long long)N);
  if (boundary < VW_PERIODIC || boundary > VW_ZERO_PADDING)
    return fail(VW_ERR_BOUNDARY, "MODWT only supports PERIODIC, ZERO_PADDING, and SYMMETRIC boundary modes");
  if (L < 1 || L > kMaxTaps) return fail(VW_ERR_ARG, "filter length %d unsupported (1..%d)", L, kMaxTaps);
  return VW_OK;
}

inline vw_status check_levels(int64_t N, int L, int J, unsigned flags) {
  if (flags & VW_FLAG_CORE_LEVELS) {
    const int maxl = max_levels(N, L);
    if (J < 1 || J > maxl)
      return fail(VW_ERR_LEVEL, "Invalid number of decomposition levels: %d (valid 1..%d for N=%lld, L=%d)", J, maxl,
                  (long long)N, L);
  } else {
    if (J < 1) return fail(VW_ERR_LEVEL, "levels must be >= 1");
    if (J > kMaxLevels) return fail(VW_ERR_LEVEL, "levels %d exceeds engine limit %d", J, kMaxLevels);
    if (upsampled_length(L, J) > (int64_t)1 << 30) return fail(VW_ERR_TOO_LARGE, "upsampled filter too long");
  }
  return VW_OK;
}

// The _bi_ entry points (two filter lengths; Lhi == 0: an equal-length entry point, nothing to check).  L has
// passed check_common / check_levels, which for CORE_LEVELS is the reference's cap on the low-pass length alone
// (calculateMaxLevels :455-501); its guards then want both upsampled filters within the signal (:717-729,
// :561-574).  Without CORE_LEVELS the longer filter meets the equal-length call's checks.
inline vw_status check_bank(int64_t N, int L, int Lhi, int J, unsigned flags, bool forward) {
  if (Lhi == 0) return VW_OK;
  if (Lhi < 1 || Lhi > kMaxTaps) return fail(VW_ERR_ARG, "filter length %d unsupported (1..%d)", Lhi, kMaxTaps);
  if (flags & VW_FLAG_CORE_LEVELS) {
    if (upsampled_length(std::max(L, Lhi), J) > N)
      return fail(VW_ERR_TOO_LARGE, "Upsampled %s filter length exceeds signal length", forward ? "analysis" : "reconstruction");
  } else if (forward && Lhi > L) {
    if (upsampled_length(Lhi, J) > (int64_t)1 << 30) return fail(VW_ERR_TOO_LARGE, "upsampled filter too long");
  }
  return VW_OK;
}

// The argument checks of vw_modwt_forward_*, in its order, on a call whose outputs are `out` and `out2` (energy
// and multiresolution calls have the one: they pass it twice).
template <typename T>
vw_status check_forward(vw_ctx* c, const FwdCall<T>& k, const void* out, const void* out2) {
  VW_TRY(check_common(c, k.x, out, k.lo, k.hi, k.B, k.N, k.L, k.boundary));
  if (!out2) return fail(VW_ERR_NULL, "approx is null");
  if (k.ldx < k.N) return fail(VW_ERR_ARG, "ldx (%lld) < N (%lld)", (long long)k.ldx, (long long)k.N);
  VW_TRY(check_levels(k.N, k.L, k.J, k.flags));
  return check_bank(k.N, k.L, k.Lhi, k.J, k.flags, true);
}

// ... and of vw_modwt_inverse_* (shared with the multiresolution calls, which make them too).
inline vw_status check_inverse_levels(int64_t N, int L, int J, unsigned flags) {
  if (J < 1 || J > kMaxLevels) return fail(VW_ERR_LEVEL, "levels must be in 1..%d", kMaxLevels);
  // applyScaledInverseMODWT guard :561-574 (reconstruct has no level cap, only L_j <= N); the SWT
  // periodic inverse (VectorWaveSwtAdapter.reconstructPeriodic :444-474) wraps instead.
  if ((flags & VW_FLAG_CORE_LEVELS) && upsampled_length(L, J) > N)
    return fail(VW_ERR_TOO_LARGE, "Upsampled reconstruction filter length exceeds signal length");
  return VW_OK;
}

template <typename T>
vw_status check_inverse(vw_ctx* c, const InvCall<T>& k) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  if (!k.y || !k.lo || !k.hi) return fail(VW_ERR_NULL, "null argument");
  if (!k.details && k.detail_mask) return fail(VW_ERR_NULL, "details is null");
  if (!k.approx && !k.approx_zero) return fail(VW_ERR_NULL, "approx is null");
  VW_TRY(check_common(c, k.y, k.y, k.lo, k.hi, k.B, k.N, k.L, k.boundary));
  VW_TRY(check_inverse_levels(k.N, k.L, k.J, k.flags));
  return check_bank(k.N, k.L, k.Lhi, k.J, k.flags, false);
}

// Validation, and any call that synchronizes, cannot be recorded into a graph (vw_capture_begin).
inline vw_status capture_guard(vw_ctx* c, unsigned flags) {
  if (c->capturing && (flags & (VW_FLAG_VALIDATE | VW_FLAG_HOST_MEMORY | VW_FLAG_SYNC)))
    return fail(VW_ERR_STATE, "validation, host memory and SYNC cannot be captured");
  return VW_OK;
}

// ------------------------------------------------------------------------------------------------
// The call records (vw_plan.h), built once at the extern "C" boundary from the ABI's common prefix; what an entry
// point adds (detail_mask, thresholds, single_level, ...) it sets on the result.
template <typename T>
FwdCall<T> fwd_call(const T* x, int64_t B, int64_t N, int64_t ldx, const double* lo, const double* hi, int L,
                    int boundary, int J, unsigned flags, T* details, T* approx, int Lhi = 0) {
  FwdCall<T> k;
  k.x = x; k.B = B; k.N = N; k.ldx = ldx; k.lo = lo; k.hi = hi; k.L = L; k.boundary = boundary; k.J = J;
  k.flags = flags; k.details = details; k.approx = approx; k.Lhi = Lhi;
  return k;
}

template <typename T>
InvCall<T> inv_call(const T* details, const T* approx, int64_t B, int64_t N, const double* lo, const double* hi,
                    int L, int wid, int boundary, int J, unsigned flags, T* y, int Lhi = 0) {
  InvCall<T> k;
  k.details = details; k.approx = approx; k.B = B; k.N = N; k.lo = lo; k.hi = hi; k.L = L; k.wid = wid;
  k.boundary = boundary; k.J = J; k.flags = flags; k.y = y; k.Lhi = Lhi;
  return k;
}

// The inverse of a forward's coefficients into y, same bank and flags (a single-level forward: the pairwise sums).
template <typename T>
InvCall<T> inverse_of(const FwdCall<T>& f, T* y, int wid = VW_WID_OTHER) {
  InvCall<T> k = inv_call<T>(f.details, f.approx, f.B, f.N, f.lo, f.hi, f.L, wid, f.boundary, f.J, f.flags, y, f.Lhi);
  k.single_level = f.single_level;
  if (f.single_level) k.detail_mask = 1u;
  return k;
}

template <typename T>
void copy_taps(T* dst, const double* src, int L) {
  // base taps * (1.0 / Math.sqrt(2.0)) in double, then rounded to T  (ScalarOps.java:911-914)
  const double s = 1.0 / std::sqrt(2.0);
  for (int i = 0; i < L; ++i) dst[i] = (T)(src[i] * s);
  for (int i = L; i < kMaxTaps; ++i) dst[i] = T(0);
}

// Both filters of a call for a kernel of `taps` taps (the plan's, vw_plan.h): a bank of two lengths has its shorter
// filter zero-extended, and on the pairwise inverses (taps = k.L) a longer high-pass truncated.
template <typename T, typename Call>
void copy_bank(T* lo, T* hi, const Call& k, int taps, int taps_hi = 0) {
  copy_taps(lo, k.lo, std::min(k.L, taps));
  copy_taps(hi, k.hi, std::min(k.Lhi > 0 ? k.Lhi : k.L, taps_hi > 0 ? taps_hi : taps));
}

// ------------------------------------------------------------------------------------------------
// The executors (vw_exec.cpp): plan, reserve, launch, fix up.  Device pointers; the caller holds the context.
template <typename T>
vw_status forward_impl(vw_ctx* c, FwdCall<T> k);
template <typename T>
vw_status inverse_impl(vw_ctx* c, InvCall<T> k);
// the validation word (c->bad) after the launches that wrote it; synchronizes
vw_status read_bad(vw_ctx* c, unsigned long long* out);
// VW_PAIR_FUSE (vw_exec.cpp): what a forward plan must be for its launch to become a round trip, and the round
// trip's arguments from the forward's as launched
bool pair_forward_shape(const FwdPlan<double>& p);
void pair_args(const FwdArgs<double>& f, const InvCall<double>& k, const InvPlan<double>& p, PairArgs<double>* a);

}  // namespace vw
