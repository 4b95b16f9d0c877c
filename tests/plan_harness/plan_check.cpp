// TEST INFRASTRUCTURE: walks a matrix of calls and tunings through the planner (vectorwave_amd/csrc/vw_plan.cpp,
// linked without anything from HIP) and checks every plan against the kernels' launch contracts, then compares
// the pinned configurations and the padded-layout rule (blk_pad) with its table of values.  Prints nothing when all is well; otherwise one line per finding: the call, the
// plan as text and the broken rule.  tests/test_plan_cpu.py fails on any output.
//   plan_check                      the whole matrix and the pins
//   plan_check show fwd|inv f64|f32 B N L J boundary flags [wid] [VW_KEY=value ...] [x+8 d+8 a+8 y+8 t+8 ldx=N+3]
//                                   one plan as text; x / d / a / y / t + bytes: the caller's x, details, approx, y and
//                                   thresholds that many bytes off a 16-byte boundary (t+ also passes thresholds),
//                                   ldx=: the forward input's leading dimension, mask=: the inverse's detail mask,
//                                   az=1: approx_zero with approx = NULL, Lhi=: a two-length bank's high-pass tap
//                                   count, single=1: the single-level entry points
#include "../../vectorwave_amd/csrc/vw_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace vw;

static int g_findings = 0;

struct TuneSet {
  const char* name;
  std::vector<std::pair<const char*, int>> kv;
};
static const std::vector<TuneSet> kTunings = {
    {"default", {}},
    {"VW_BLK=0", {{"VW_BLK", 0}}},
    {"VW_INV_BUF=1", {{"VW_INV_BUF", 1}}},
    {"VW_INV_BUF=2", {{"VW_INV_BUF", 2}}},
    {"VW_NV=8", {{"VW_NV", 8}}},
    {"VW_FWD_NV=2", {{"VW_FWD_NV", 2}}},
    {"VW_INV_NV=2", {{"VW_INV_NV", 2}}},
    {"VW_FWD_PERSIST=0", {{"VW_FWD_PERSIST", 0}}},
    {"VW_FORCE_TILED=1", {{"VW_FORCE_TILED", 1}}},
    {"VW_FORCE_TILED=1 VW_MULTI_TILE=256", {{"VW_FORCE_TILED", 1}, {"VW_MULTI_TILE", 256}}},
    {"VW_FORCE_TILED=1 VW_MULTI_TILE=512", {{"VW_FORCE_TILED", 1}, {"VW_MULTI_TILE", 512}}},
    {"VW_DEEP=1", {{"VW_DEEP", 1}}},
    {"VW_SWEEP2=0 VW_SWEEP2_MINB=1", {{"VW_SWEEP2", 0}, {"VW_SWEEP2_MINB", 1}}},
    {"VW_SWEEP2=2 VW_SWEEP2_MINB=1", {{"VW_SWEEP2", 2}, {"VW_SWEEP2_MINB", 1}}},
    {"VW_SWEEP2=3 VW_SWEEP2_MINB=1", {{"VW_SWEEP2", 3}, {"VW_SWEEP2_MINB", 1}}},
    {"VW_MULTI_NI=4", {{"VW_MULTI_NI", 4}}},
    {"VW_MULTI_NI=8", {{"VW_MULTI_NI", 8}}},
    {"VW_MULTI_PAD=0", {{"VW_MULTI_PAD", 0}}},
    {"VW_LEVEL_CT=0", {{"VW_LEVEL_CT", 0}}},
    {"VW_MFMA=3", {{"VW_MFMA", 3}}},
    {"VW_BLK_FWD8=0", {{"VW_BLK_FWD8", 0}}},
};

static Tuning make_tuning(const TuneSet& ts) {
  Tuning t;
  for (const auto& kv : ts.kv)
    if (!set_tuning(t, kv.first, kv.second)) {
      printf("unknown tuning switch %s\n", kv.first);
      ++g_findings;
    }
  return t;
}

// ------------------------------------------------------------------------------------------------
// A plan as one line of text (also the form of the pins).
static const char* const kKernelNames[] = {"fused",  "persist", "blk",   "mfma",   "pair",  "seq",  "db",
                                           "blk",    "mfma",    "deep",  "multi",  "sweepg", "sweep", "tile"};
static const char* const kBufNames[] = {"none", "in", "ws0", "ws1", "out"};

template <typename T, typename Args>
static std::string describe(const Plan<T, Args>& p, bool inverse) {
  char b[256];
  if (p.error != VW_OK) {
    snprintf(b, sizeof(b), "error %d (%s)", p.error, p.msg);
    return b;
  }
  std::string s = inverse ? "inv " : "fwd ";
  if (p.fused) {
    snprintf(b, sizeof(b), "%s threads=%d nv=%d lds=%d", kKernelNames[p.kernel], p.threads, p.nv, p.lds);
    s += b;
  } else {
    s += "levels:";
    for (const auto& st : p.steps) {
      snprintf(b, sizeof(b), " %s[%d-%d %s>%s lds=%d", kKernelNames[st.kind], st.jlo, st.jhi, kBufNames[st.src],
               kBufNames[st.dst], st.lds);
      s += b;
      if (st.kind == kStepMulti) snprintf(b, sizeof(b), " tile=%d ni=%d pad=%d]", st.multi.tile, st.multi.ni, st.multi.pad);
      else if (st.kind == kStepDeep) snprintf(b, sizeof(b), " seg=%d]", st.deep.seg);
      else if (st.kind == kStepSweepG) snprintf(b, sizeof(b), " G=%d ka=%d R=%d tile=%d]", st.G, st.ka, st.R, st.lvl.tile);
      else snprintf(b, sizeof(b), " tile=%d]", st.lvl.tile);
      s += b;
    }
  }
  snprintf(b, sizeof(b), " ref_nf=%d probed=%d ws=%zu nf_rows=%lld ref_grid=%d", (int)p.ref_nf, (int)p.nf_probed,
           p.res.ws_bytes, (long long)p.res.nf_rows, p.res.ref_grid);
  s += b;
  return s;
}
struct Ctx {  // what a finding prints
  const char* dir;
  const char* dtype;
  const char* tune;
  long long B, N, ld;
  int L, J, boundary, wid;
  unsigned flags;
  const char* extra;
};
static void finding(const Ctx& c, const std::string& plan, const char* rule) {
  if (++g_findings > 200) return;  // enough to read
  printf("%s %s B=%lld N=%lld ld=%lld L=%d J=%d boundary=%d wid=%d flags=0x%x %s [%s] | %s | %s\n", c.dir, c.dtype,
         c.B, c.N, c.ld, c.L, c.J, c.boundary, c.wid, c.flags, c.extra, c.tune, plan.c_str(), rule);
}

// ------------------------------------------------------------------------------------------------
// The rules.
template <typename T> static constexpr int vecw() { return 16 / (int)sizeof(T); }
static bool plus_zero(const LevelDesc& d) { return d.dir_a == 1 && d.dir_d == 1 && d.off_a == 0 && d.off_d == 0; }

// Rule 8, alignment: what the kernels' loads and stores need, read from their code, not from the planner's conditions.
//   - store_vec / load_row_regs / tile_to_lds take the 16-byte path when vec_ok, and the tap-unrolled fused kernels
//     set vec_ok = (L > 0) || vec_io: `unrolled`, `full` and `vec_io` all mean 16-byte accesses at row + w * V.
//   - k_forward_persist (LDS-DMA of 16 bytes per lane from x + b * ldx), the register-blocked and matrix-core
//     kernels have no scalar form at all.
//   - the deep kernels (vw_deep.hip) feed their rings by 16-byte DMA and store whole vectors; k_*_multi and
//     k_*_level follow their own vec_io, and k_inverse_multi's prefetch / padded layout (pf, pad) loads vectors
//     unconditionally.
//   - the column sweeps and the chained sweeps (k_*_sweep, k_inverse_sweep2 / 3) load and store single elements:
//     they need nothing.
// A row of a caller array starts at base + b * ld (+ k * B * N for plane k of the details), so base % 16 == 0 with
// ld % V == 0 and N % V == 0 is what makes every row a whole number of vectors from a 16-byte boundary; the workspace
// halves (256-byte aligned base, second half one plane on) need N % V == 0 alone.
static bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

struct Ptrs {  // the caller pointers of one call, as the steps' buffer names see them
  const void* in;       // forward x, inverse approx (nullptr: none)
  long long ld_in;      // leading dimension of `in`
  const void* out;      // forward approx, inverse y
  const void* details;
  long long B, N;
  int elem;
};
static bool buf_ok(const Ptrs& q, int b, bool first_level_input) {
  const int V = 16 / q.elem;
  if (b == kBufIn) return (!q.in || al16(q.in)) && (!first_level_input || q.ld_in % V == 0);
  if (b == kBufOut) return al16(q.out);
  return true;  // workspace halves: N % V == 0, checked by the caller
}
static bool plane_ok(const Ptrs& q, int k) { return al16((const char*)q.details + (size_t)k * q.B * q.N * q.elem); }

template <typename T, typename Args>
static const char* check_step_alignment(const Plan<T, Args>& p, bool inverse, const Ptrs& q) {
  constexpr int V = vecw<T>();
  for (const auto& s : p.steps) {
    bool vec = false;
    switch (s.kind) {
      case kStepDeep: vec = true; break;
      case kStepMulti:
        if ((s.multi.pf || s.multi.pad) && !s.multi.vec_io) return "8: multi-level prefetch / padded layout without vec_io";
        vec = s.multi.vec_io != 0;
        break;
      case kStepTile: vec = s.lvl.vec_io != 0; break;
      default: break;  // sweeps: element accesses only
    }
    if (!vec) continue;
    if (q.N % V) return "8: vector I/O on rows that are no whole number of vectors";
    if (!buf_ok(q, s.src, !inverse)) return "8: vector loads from a misaligned input (or leading dimension)";
    if (!buf_ok(q, s.dst, false)) return "8: vector stores to a misaligned output";
    for (int j = s.jlo; j <= s.jhi; ++j)
      if ((!inverse || p.args.lv[j - 1].use_d) && !plane_ok(q, j - 1)) return "8: vector I/O on a misaligned detail plane";
  }
  return nullptr;
}

// rules 1, 2, 5 and 7 on the per-level path (both directions)
template <typename T, typename Args>
static const char* check_steps(const Plan<T, Args>& p, bool inverse, int L, int J, long long B, long long N) {
  if (p.steps.empty()) return "5: no steps";
  int next = inverse ? J : 1;
  int prev_dst = -1;
  bool ws = false;
  for (const auto& s : p.steps) {
    if (s.jlo > s.jhi || (inverse ? s.jhi : s.jlo) != next) return "5: levels not covered once, in order";
    next = inverse ? s.jlo - 1 : s.jhi + 1;
    if (s.src == s.dst) return "5: a step reads the buffer it writes";
    if (prev_dst >= 0 && s.src != prev_dst) return "5: a step does not read what the last one wrote";
    if (prev_dst < 0 && s.src != kBufIn && !(inverse && s.src == kBufNone)) return "5: first step does not read the caller's input";
    if (s.src == kBufOut || s.dst == kBufIn || s.dst == kBufNone) return "5: caller buffers misused";
    prev_dst = s.dst;
    ws = ws || s.dst == kBufWs0 || s.dst == kBufWs1;
    const int g = s.jhi - s.jlo + 1;
    if (s.lds > kLdsBytes) return "2: LDS bytes";
    switch (s.kind) {
      case kStepDeep:
        if (!has_unrolled_taps(L)) return "1: deep group at an unlisted length";
        if (g > kMaxGroup || s.deep.g != g) return "2: deep group size";
        break;
      case kStepMulti:
        if (g > kMaxGroup || g < 2 || s.multi.nlev != g) return "2: multi-level group size";
        if (inverse && s.multi.pad && !has_unrolled_taps(L)) return "1: padded multi-level layout at an unlisted length";
        break;
      case kStepSweepG: {
        if (!has_unrolled_taps(L)) return "1: chained sweep at an unlisted length";
        const long long rings = (s.G == 2 ? 1 : 2) * 3LL * s.G * s.ka * s.R * (long long)sizeof(T);
        if (!inverse || (s.G != 2 && s.G != 4) || g != (s.G == 2 ? 2 : 3) || rings > kLdsBytes) return "2: chained sweep shape";
        break;
      }
      case kStepSweep:
        if (!has_unrolled_taps(L)) return "1: sweep at an unlisted length";
        if (g != 1) return "5: sweep over more than one level";
        break;
      case kStepTile:
        if (g != 1) return "5: tile over more than one level";
        break;
      default:
        return "5: unknown step kind";
    }
    if (s.probe && !p.ref_nf) return "6: probe without the fix-up";
  }
  if (next != (inverse ? 0 : J + 1)) return "5: levels not covered to the end";
  if (prev_dst != kBufOut) return "5: last step does not write the caller's output";
  const auto& last = p.steps.back();
  if (p.nf_probed != (last.probe != 0)) return "6: nf_probed is not the last step's probe";
  if (last.probe && last.kind != (inverse ? kStepMulti : kStepDeep)) return "6: probing step is not a probing kernel";
  for (size_t i = 0; i + 1 < p.steps.size(); ++i)
    if (p.steps[i].probe) return "6: a step before the last probes";
  if (ws && p.res.ws_bytes < 2 * (size_t)B * (size_t)N * sizeof(T)) return "7: workspace planes not reserved";
  return nullptr;
}

template <typename T, typename Args>
static const char* check_reserve(const Plan<T, Args>& p, long long B, long long N) {
  if (p.nf_probed && !p.ref_nf) return "6: probed without the fix-up";
  if (!p.ref_nf) return p.res.ref_grid ? "7: fix-up grid without a fix-up" : nullptr;
  if (p.res.nf_rows < B) return "7: row flags not reserved";
  if (p.res.ref_grid < 1 || p.res.ref_grid > B) return "7: fix-up grid";
  if (p.res.ws_bytes < (size_t)p.res.ref_grid * 2 * (size_t)N * sizeof(T)) return "7: fix-up scratch not reserved";
  return nullptr;
}

template <typename T>
static const char* check_forward(const FwdCall<T>& c, const FwdPlan<T>& p) {
  constexpr int V = vecw<T>();
  if (p.error == VW_ERR_UNSUPPORTED) return nullptr;  // a refusal with a reason is a valid answer
  if (p.error != VW_OK) return "plan error";
  const long long nvec = (c.N + V - 1) / V;
  const bool may_ref = (c.flags & VW_FLAG_REF_NONFINITE) && !(c.flags & VW_FLAG_VALIDATE) && !c.single_level &&
                       c.J >= 2 && !(c.flags & VW_FLAG_FFT_SWITCH) &&
                       !(c.hist && c.hist_update && !c.hist_first && !c.hist_snap);
  if (p.ref_nf != may_ref) return "6: fix-up where excluded (or missing)";
  if (const char* r = check_reserve(p, c.B, c.N)) return r;
  const Ptrs q{c.x, c.ldx, c.approx, c.details, c.B, c.N, (int)sizeof(T)};
  if (!p.fused) {
    if (const char* r = check_steps(p, false, c.L, c.J, c.B, c.N)) return r;
    return check_step_alignment(p, false, q);
  }
  const FwdArgs<T>& a = p.args;
  if (a.vec_io || a.unrolled || p.kernel == kFwdPersist || p.kernel == kFwdBlk || p.kernel == kFwdMfma) {
    if (c.N % V || c.ldx % V) return "8: vector I/O on rows that are no whole number of vectors";
    if (!al16(c.x) || !al16(c.approx)) return "8: vector I/O on a misaligned x / approx";
    for (int j = 0; j < c.J; ++j)
      if (!plane_ok(q, j)) return "8: vector I/O on a misaligned detail plane";
  }
  if (p.lds > kLdsBytes || p.lds <= 0) return "2: LDS bytes";
  if (p.threads > kMaxThreads || p.threads < 1) return "2: threads";
  if (c.J > kMaxLevels) return "2: levels on the fused path";
  if (p.kernel != kFwdMfma && (long long)p.threads * p.nv < nvec) return "2: workgroup does not cover the row";
  if (p.nv == 2 && !(has_unrolled_taps(c.L) && c.L <= 8 && a.unrolled)) return "1: NV = 2 without an unrolled kernel";
  if (p.nv == 2 && (long long)p.threads * 2 != nvec) return "1: NV = 2 without full slabs";
  const bool periodic = [&] { for (int j = 0; j < c.J; ++j) if (a.lv[j].mode != kHaloPeriodic) return false; return true; }();
  switch (p.kernel) {
    case kFwdFused:
      break;
    case kFwdPersist:
      if (!has_unrolled_taps(c.L)) return "1: persistent forward at an unlisted length";
      if (!a.region1 || p.nv != 4 || (long long)p.threads * p.nv != nvec || p.threads % 64 || nvec % 64 || !a.vec_io ||
          !a.unrolled || p.validate || c.hist)
        return "3: persistent forward's contract";
      break;
    case kFwdBlk: {
      if (!has_unrolled_taps(c.L)) return "1: blocked forward at an unlisted length";
      const int mJ = std::max(1, a.lv[c.J - 1].s / V);
      if (!periodic || (long long)p.threads * p.nv != nvec || nvec % ((long long)p.nv * mJ) || p.nv == 2 || !a.unrolled ||
          p.validate || c.hist || a.hlpad / V > nvec)
        return "4: blocked forward's contract";
      break;
    }
    case kFwdMfma:
      if (!std::is_same<T, float>::value || !mfma_supported(c.L, c.N) || !periodic || !p.fma || !a.vec_io)
        return "1: matrix-core forward outside its instantiations";
      break;
    default:
      return "unknown forward kernel";
  }
  const bool probing = p.kernel == kFwdPersist || p.kernel == kFwdBlk;
  if (p.nf_probed && !probing) return "6: probed by a kernel that does not probe";
  return nullptr;
}

template <typename T>
static const char* check_inverse(const InvCall<T>& c, const InvPlan<T>& p) {
  constexpr int V = vecw<T>();
  if (p.error == VW_ERR_UNSUPPORTED) return nullptr;
  if (p.error != VW_OK) return "plan error";
  const long long nvec = (c.N + V - 1) / V;
  const bool may_ref = (c.flags & VW_FLAG_REF_NONFINITE) && !c.single_level && c.J >= 2;
  if (p.ref_nf != may_ref) return "6: fix-up where excluded (or missing)";
  if (const char* r = check_reserve(p, c.B, c.N)) return r;
  const Ptrs q{c.approx_zero ? nullptr : c.approx, c.N, c.y, c.details, c.B, c.N, (int)sizeof(T)};
  if (!p.fused) {
    if (const char* r = check_steps(p, true, c.L, c.J, c.B, c.N)) return r;
    return check_step_alignment(p, true, q);
  }
  const InvArgs<T>& a = p.args;
  if (a.vec_io || a.unrolled || a.full || a.blk || p.kernel == kInvBlk || p.kernel == kInvMfma) {
    if (c.N % V) return "8: vector I/O on rows that are no whole number of vectors";
    if (!al16(c.y) || (q.in && !al16(q.in))) return "8: vector I/O on a misaligned approx / y";
    for (int j = 0; j < c.J; ++j)
      if (a.lv[j].use_d && !plane_ok(q, j)) return "8: vector I/O on a misaligned detail plane";
  }
  if (p.lds > kLdsBytes || p.lds <= 0) return "2: LDS bytes";
  if (p.threads > kMaxThreads || p.threads < 1) return "2: threads";
  if (c.J > kMaxLevels) return "2: levels on the fused path";
  if (p.kernel != kInvMfma && (long long)p.threads * p.nv < nvec) return "2: workgroup does not cover the row";
  if (p.nv == 2 && !(has_unrolled_taps(c.L) && c.L <= 8 && a.unrolled)) return "1: NV = 2 without an unrolled kernel";
  if (p.nv == 2 && (long long)p.threads * 2 != nvec) return "1: NV = 2 without full slabs";
  const bool pair = c.single_level || c.boundary == VW_ZERO_PADDING;
  if ((a.pair != 0) != pair) return "pairwise sums where the reference has sequential ones (or the reverse)";
  bool pz = true;
  for (int j = 0; j < c.J; ++j) pz = pz && a.lv[j].mode == kHaloPeriodic && plus_zero(a.lv[j]);
  // the full-slab form of k_inverse_seq (listed lengths up to 8 at NV = 4: the launcher's own dispatch) needs
  // aligned rows and threads * NV == nvec wherever the flag is set
  if (a.full && !(a.vec_io && a.unrolled && (long long)p.threads * p.nv == nvec))
    return "1: full-slab flag without full slabs";
  switch (p.kernel) {
    case kInvPair: if (!a.pair || a.blk) return "pair kernel without pairwise sums"; break;
    case kInvSeq: if (a.pair || a.db || a.blk) return "seq kernel with other flags"; break;
    case kInvDb: if (a.pair || !a.db || a.blk) return "db kernel with other flags"; break;
    case kInvBlk: {
      if (!has_unrolled_taps(c.L)) return "1: blocked inverse at an unlisted length";
      const int mJ = std::max(1, a.lv[c.J - 1].s / V);
      if (!pz || a.pair || a.db || !a.blk || p.nv == 2 || !a.unrolled || (long long)p.threads * p.nv != nvec ||
          nvec % ((long long)p.nv * mJ))
        return "4: blocked inverse's contract";
      break;
    }
    case kInvMfma:
      if (!std::is_same<T, float>::value || !mfma_supported(c.L, c.N) || !pz || !p.fma || !a.vec_io || a.pair)
        return "1: matrix-core inverse outside its instantiations";
      break;
    default:
      return "unknown inverse kernel";
  }
  if (p.kernel != kInvBlk && p.kernel != kInvMfma && a.blk) return "4: blk flag on another kernel";
  const bool probing = p.kernel == kInvSeq || p.kernel == kInvBlk;
  if (p.nf_probed && !probing) return "6: probed by a kernel that does not probe";
  return nullptr;
}

// ------------------------------------------------------------------------------------------------
// The matrix.
template <typename T> static const char* dtype_name() { return sizeof(T) == 8 ? "f64" : "f32"; }
template <typename T> static T* fake(uintptr_t v) { return reinterpret_cast<T*>(v); }  // never dereferenced

enum { kOffX = 1, kOffDetails = 2, kOffApprox = 4, kOffY = 8, kOffThr = 16 };

struct Axes {  // everything beyond (dtype, L, boundary, N, J, B)
  unsigned flags = 0;
  int misalign = 0;      // mask of the caller pointers one element off a 16-byte boundary: kOffX ...
  int ld_extra = 0;      // ldx = N + ld_extra
  int hist = 0;          // 0 none, 1 read only (flush), 2 update, 3 update + snapshot, 4 update, first block
  bool thr = false;
  unsigned mask = ~0u;
  bool single = false;
  int wid = VW_WID_OTHER;
  const char* name = "";
};

template <typename T>
static void run_case(const TuneSet& ts, const Tuning& tu, long long B, long long N, int L, int J, int boundary,
                     const Axes& ax) {
  static T* hist_ptrs[kMaxLevels];
  for (int j = 0; j < kMaxLevels; ++j) hist_ptrs[j] = fake<T>(0x900000 + 0x1000 * j);
  if (ax.single) J = 1;
  Ctx ctx{"fwd", dtype_name<T>(), ts.name, B, N, N + ax.ld_extra, L, J, boundary, ax.wid, ax.flags, ax.name};
  {
    FwdCall<T> c;
    auto off = [&](int bit) { return (ax.misalign & bit) ? sizeof(T) : 0; };
    c.x = fake<T>(0x100000 + off(kOffX)); c.details = fake<T>(0x200000 + off(kOffDetails));
    c.approx = fake<T>(0x300000 + off(kOffApprox));
    c.B = B; c.N = N; c.ldx = N + ax.ld_extra; c.L = L; c.boundary = boundary; c.J = J;
    c.flags = ax.single ? ax.flags & ~VW_FLAG_FFT_SWITCH : ax.flags;
    c.single_level = ax.single;
    if (ax.hist && boundary != VW_PERIODIC && !ax.single) {  // streaming blocks: ZERO / SYMMETRIC only
      c.hist = hist_ptrs; c.mode_override = kHaloHistory;
      c.hist_update = ax.hist >= 2; c.hist_snap = ax.hist == 3 ? hist_ptrs : nullptr; c.hist_first = ax.hist == 4;
    }
    FwdPlan<T> p;
    plan_forward(tu, c, &p);
    if (const char* r = check_forward(c, p)) finding(ctx, describe(p, false), r);
  }
  {
    InvCall<T> c;
    auto off = [&](int bit) { return (ax.misalign & bit) ? sizeof(T) : 0; };
    c.details = fake<T>(0x200000 + off(kOffDetails)); c.approx = fake<T>(0x300000 + off(kOffApprox));
    c.y = fake<T>(0x400000 + off(kOffY));
    c.B = B; c.N = N; c.L = L; c.wid = ax.wid; c.boundary = boundary; c.J = J;
    c.flags = ax.flags & ~(VW_FLAG_VALIDATE | VW_FLAG_FFT_SWITCH);
    c.detail_mask = ax.single ? 1u : ax.mask; c.single_level = ax.single;
    if (ax.thr) { c.thr = fake<T>(0x500000 + off(kOffThr)); c.soft = 1; c.thr_ld = B; }
    InvPlan<T> p;
    plan_inverse(tu, c, &p);
    ctx.dir = "inv";
    if (const char* r = check_inverse(c, p)) finding(ctx, describe(p, true), r);
  }
}

static const long long kNs[] = {7, 64, 512, 1000, 4096, 8192, 16384, 65536, 1 << 20};
static const long long kBs[] = {1, 512, 513, 4096};
static const int kBoundaries[] = {VW_PERIODIC, VW_SYMMETRIC, VW_ZERO_PADDING};

// J in {1, 2, 6, the largest the level check admits up to 10}: without VW_FLAG_CORE_LEVELS that is 10 for every
// L <= 64 (the upsampled filter stays far below 2^30 taps); with it, max_levels(N, L) where that is >= 1.
static std::vector<int> levels_of(long long N, int L) {
  std::vector<int> js = {1, 2, 6, 10};
  const int core = max_levels(N, L);
  if (core >= 1 && core != 1 && core != 2 && core != 6 && core != 10) js.push_back(core);
  return js;
}

template <typename T>
static void run_matrix() {
  std::vector<Axes> rest;
  {
    Axes a;
    a.flags = VW_FLAG_FMA; a.name = "fma"; rest.push_back(a);
    a.flags = VW_FLAG_VALIDATE; a.name = "validate"; rest.push_back(a);
    a.flags = VW_FLAG_REF_NONFINITE; a.name = "ref_nf"; rest.push_back(a);
    a.flags = VW_FLAG_REF_NONFINITE | VW_FLAG_FMA; a.name = "ref_nf+fma"; rest.push_back(a);
    a.flags = VW_FLAG_REF_NONFINITE | VW_FLAG_VALIDATE; a.name = "ref_nf+validate"; rest.push_back(a);
    a.flags = VW_FLAG_FFT_SWITCH; a.name = "fft"; rest.push_back(a);
    a.flags = VW_FLAG_FFT_SWITCH | VW_FLAG_REF_NONFINITE; a.name = "fft+ref_nf"; rest.push_back(a);
    // every caller pointer alone, and all together, one element off a 16-byte boundary
    static const struct { int mask; const char* name; } kOffsets[] = {
        {kOffX, "x+1"}, {kOffDetails, "details+1"}, {kOffApprox, "approx+1"}, {kOffY, "y+1"}, {kOffThr, "thr+1"},
        {kOffX | kOffDetails | kOffApprox | kOffY | kOffThr, "all+1"}};
    for (const auto& o : kOffsets) {
      a = Axes(); a.misalign = o.mask; a.thr = (o.mask & kOffThr) != 0; a.name = o.name; rest.push_back(a);
    }
    a = Axes(); a.misalign = kOffX | kOffApprox; a.flags = VW_FLAG_REF_NONFINITE; a.name = "x+1 approx+1 ref_nf"; rest.push_back(a);
    a = Axes(); a.misalign = kOffDetails; a.mask = 0x15u; a.name = "details+1 mask"; rest.push_back(a);
    a = Axes(); a.ld_extra = 1; a.name = "ldx=N+1"; rest.push_back(a);
    for (int h = 1; h <= 4; ++h)
      for (unsigned f : {0u, (unsigned)VW_FLAG_REF_NONFINITE}) {
        a = Axes(); a.hist = h; a.flags = f;
        static const char* const names[] = {"", "hist flush", "hist update", "hist update+snap", "hist first"};
        a.name = names[h]; rest.push_back(a);
      }
    a = Axes(); a.thr = true; a.name = "thr"; rest.push_back(a);
    a.flags = VW_FLAG_REF_NONFINITE; a.name = "thr ref_nf"; rest.push_back(a);
    a = Axes(); a.mask = 0x15u; a.name = "mask"; rest.push_back(a);
    a.flags = VW_FLAG_REF_NONFINITE; a.name = "mask ref_nf"; rest.push_back(a);
    a = Axes(); a.single = true; a.name = "single"; rest.push_back(a);
    a.flags = VW_FLAG_REF_NONFINITE | VW_FLAG_FMA; a.name = "single ref_nf+fma"; rest.push_back(a);
    a = Axes(); a.single = true; a.flags = VW_FLAG_BATCH_SYM_INVERSE; a.name = "single batch-sym"; rest.push_back(a);
    for (int wid : {VW_WID_DB4, VW_WID_DB6, VW_WID_DB8, VW_WID_SYM4, VW_WID_SYM8, VW_WID_COIF2, VW_WID_COIF3, VW_WID_COIF5}) {
      a = Axes(); a.wid = wid; a.name = "wid"; rest.push_back(a);
    }
  }
  static const int kRestL[] = {3, 8, 16, 22, 30, 31, 64};
  const Axes plain;
  for (const TuneSet& ts : kTunings) {
    const Tuning tu = make_tuning(ts);
    for (int boundary : kBoundaries)
      for (long long N : kNs)
        for (long long B : kBs) {
          for (int L = 1; L <= 64; ++L)
            for (int J : levels_of(N, L)) run_case<T>(ts, tu, B, N, L, J, boundary, plain);
          for (int L : kRestL)
            for (int J : levels_of(N, L))
              for (const Axes& ax : rest) run_case<T>(ts, tu, B, N, L, J, boundary, ax);
        }
  }
}

// ------------------------------------------------------------------------------------------------
// Pins: exact expected plans (pins.inc; the values come from launch traces of the kernels, not from the planner).
struct Pin {
  const char* what;
  bool inverse;
  bool f32;
  long long B, N;
  int L, J, boundary, wid;
  unsigned flags;
  bool thr;
  const char* expect;  // describe() [+ layout() for the fp64 forward], as far as the pin goes (a prefix)
};
static const Pin kPins[] = {
#include "pins.inc"
};

static void run_pins() {
  const TuneSet& ts = kTunings[0];
  const Tuning tu = make_tuning(ts);
  for (const Pin& pin : kPins) {
    std::string got;
    auto fwd = [&](auto tag) {
      using T = decltype(tag);
      FwdCall<T> c;
      c.x = fake<T>(0x100000); c.details = fake<T>(0x200000); c.approx = fake<T>(0x300000);
      c.B = pin.B; c.N = pin.N; c.ldx = pin.N; c.L = pin.L; c.boundary = pin.boundary; c.J = pin.J; c.flags = pin.flags;
      FwdPlan<T> p;
      plan_forward(tu, c, &p);
      got = describe(p, false);
      if (p.fused) {
        char b[160];
        snprintf(b, sizeof(b), " bufs=%d hlpad=%d tap_lds=%d tight=%d unrolled=%d dma_nt=%d", p.args.region1 ? 2 : 1,
                 p.args.hlpad, p.args.tap_lds, p.args.blk_tight, p.args.unrolled, p.args.dma_nt);
        got += b;
      }
    };
    auto inv = [&](auto tag) {
      using T = decltype(tag);
      InvCall<T> c;
      c.details = fake<T>(0x200000); c.approx = fake<T>(0x300000); c.y = fake<T>(0x400000);
      c.B = pin.B; c.N = pin.N; c.L = pin.L; c.wid = pin.wid; c.boundary = pin.boundary; c.J = pin.J; c.flags = pin.flags;
      if (pin.thr) { c.thr = fake<T>(0x500000); c.soft = 1; }
      InvPlan<T> p;
      plan_inverse(tu, c, &p);
      got = describe(p, true);
      if (p.fused) {
        char b[160];
        snprintf(b, sizeof(b), " hlpad=%d tap_lds=%d tight=%d unrolled=%d full=%d", p.args.hlpad_a, p.args.tap_lds,
                 p.args.blk_tight, p.args.unrolled, p.args.full);
        got += b;
      }
    };
    if (pin.inverse) { if (pin.f32) inv(0.f); else inv(0.0); }
    else { if (pin.f32) fwd(0.f); else fwd(0.0); }
    if (got != pin.expect) {
      ++g_findings;
      printf("pin %s:\n  expected %s\n  planned  %s\n", pin.what, pin.expect, got.c_str());
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The padded layout of the register-blocked kernels (blk_pad, vw_internal.h): the planner sizes LDS with it and
// the kernels address LDS with it.  Literal values, not computed by the rule: vector stride m, outputs per
// thread nv, tight -> (shift, pad).
struct PadPin {
  int m, nv, tight, sh, pad;
};
static const PadPin kPadPins[] = {
    {0, 4, 0, 30, 0},   {0, 4, 1, 30, 0},   {0, 8, 0, 30, 0},   {0, 8, 1, 30, 0},    //
    {1, 4, 0, 2, 1},    {1, 4, 1, 2, 1},    {1, 8, 0, 3, 1},    {1, 8, 1, 4, 1},     //
    {2, 4, 0, 2, 1},    {2, 4, 1, 2, 1},    {2, 8, 0, 3, 1},    {2, 8, 1, 4, 1},     //
    {4, 4, 0, 2, 1},    {4, 4, 1, 2, 1},    {4, 8, 0, 3, 1},    {4, 8, 1, 4, 1},     //
    {8, 4, 0, 3, 2},    {8, 4, 1, 3, 2},    {8, 8, 0, 3, 1},    {8, 8, 1, 4, 1},     //
    {16, 4, 0, 30, 0},  {16, 4, 1, 30, 0},  {16, 8, 0, 30, 0},  {16, 8, 1, 30, 0},   //
    {32, 4, 0, 30, 0},  {32, 4, 1, 30, 0},  {32, 8, 0, 30, 0},  {32, 8, 1, 30, 0},   //
    {64, 4, 0, 30, 0},  {64, 4, 1, 30, 0},  {64, 8, 0, 30, 0},  {64, 8, 1, 30, 0},   //
    {128, 4, 0, 30, 0}, {128, 4, 1, 30, 0}, {128, 8, 0, 30, 0}, {128, 8, 1, 30, 0},  //
};
static_assert(blk_pad(8, 4).sh == 3 && blk_pad(8, 4).pad == 2, "blk_pad is usable in constant expressions (BlkC)");

static void run_pad_pins() {
  for (const PadPin& pin : kPadPins) {
    const BlkLayout got = blk_pad(pin.m, pin.nv, pin.tight);
    if (got.sh != pin.sh || got.pad != pin.pad) {
      ++g_findings;
      printf("blk_pad(m=%d, nv=%d, tight=%d): expected (%d, %d), got (%d, %d)\n", pin.m, pin.nv, pin.tight, pin.sh,
             pin.pad, got.sh, got.pad);
    }
  }
}

// What `show` adds to describe(): the flags that choose between a kernel's vector and element forms.
template <typename T, typename Args>
static std::string io_flags(const Plan<T, Args>& p, int full) {
  char b[96];
  if (p.error != VW_OK) return "";
  if (p.fused) {
    snprintf(b, sizeof(b), " vec_io=%d unrolled=%d full=%d", p.args.vec_io, p.args.unrolled, full);
    return b;
  }
  std::string s = " vec_io=[";
  for (const auto& st : p.steps) {
    if (s.back() != '[') s += ' ';
    s += st.kind == kStepDeep ? "1" : st.kind == kStepMulti ? (st.multi.vec_io ? "1" : "0")
         : st.kind == kStepTile ? (st.lvl.vec_io ? "1" : "0") : "-";
  }
  return s + "]";
}

template <typename T>
static int show(bool inverse, char** v, int n) {
  if (n < 6) return 2;
  Tuning tu;
  int wid = VW_WID_OTHER, az = 0, Lhi = 0, single = 0;
  long long ox = 0, od = 0, oa = 0, oy = 0, ot = -1, ldx = 0;
  unsigned mask = ~0u;
  for (int i = 6; i < n; ++i) {
    char* plus = strchr(v[i], '+');
    if (plus && plus == v[i] + 1) {  // x+8: a pointer's byte offset
      const long long o = atoll(plus + 1);
      switch (v[i][0]) {
        case 'x': ox = o; break;
        case 'd': od = o; break;
        case 'a': oa = o; break;
        case 'y': oy = o; break;
        case 't': ot = o; break;
        default: printf("unknown pointer %s\n", v[i]); return 2;
      }
      continue;
    }
    char* eq = strchr(v[i], '=');
    if (!eq) { wid = atoi(v[i]); continue; }
    *eq = '\0';
    if (!strcmp(v[i], "ldx")) { ldx = atoll(eq + 1); continue; }
    if (!strcmp(v[i], "mask")) { mask = (unsigned)strtoul(eq + 1, nullptr, 0); continue; }
    if (!strcmp(v[i], "az")) { az = atoi(eq + 1); continue; }
    if (!strcmp(v[i], "Lhi")) { Lhi = atoi(eq + 1); continue; }        // a two-length bank's high-pass taps
    if (!strcmp(v[i], "single")) { single = atoi(eq + 1); continue; }  // vw_modwt1_*: the single-level calls
    if (!set_tuning(tu, v[i], atoi(eq + 1))) { printf("unknown switch %s\n", v[i]); return 2; }
  }
  const long long B = atoll(v[0]), N = atoll(v[1]);
  const int L = atoi(v[2]), J = atoi(v[3]), boundary = atoi(v[4]);
  const unsigned flags = (unsigned)strtoul(v[5], nullptr, 0);
  if (inverse) {
    InvCall<T> c;
    c.details = fake<T>(0x200000 + od); c.approx = az ? nullptr : fake<T>(0x300000 + oa); c.y = fake<T>(0x400000 + oy);
    c.B = B; c.N = N; c.L = L; c.wid = wid; c.boundary = boundary; c.J = J; c.flags = flags;
    c.detail_mask = mask; c.approx_zero = az; c.Lhi = Lhi; c.single_level = single != 0;
    if (ot >= 0) { c.thr = fake<T>(0x500000 + ot); c.soft = 1; c.thr_ld = B; }
    InvPlan<T> p;
    plan_inverse(tu, c, &p);
    printf("%s%s\n", describe(p, true).c_str(), io_flags(p, p.args.full).c_str());
    if (const char* r = check_inverse(c, p)) { printf("%s\n", r); return 1; }
  } else {
    FwdCall<T> c;
    c.x = fake<T>(0x100000 + ox); c.details = fake<T>(0x200000 + od); c.approx = fake<T>(0x300000 + oa);
    c.B = B; c.N = N; c.ldx = ldx ? ldx : N; c.L = L; c.boundary = boundary; c.J = J; c.flags = flags;
    c.Lhi = Lhi; c.single_level = single != 0;
    FwdPlan<T> p;
    plan_forward(tu, c, &p);
    printf("%s%s\n", describe(p, false).c_str(), io_flags(p, 0).c_str());
    if (const char* r = check_forward(c, p)) { printf("%s\n", r); return 1; }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "show")) {
    const bool inverse = !strcmp(argv[2], "inv");
    return !strcmp(argv[3], "f32") ? show<float>(inverse, argv + 4, argc - 4) : show<double>(inverse, argv + 4, argc - 4);
  }
  run_matrix<double>();
  run_matrix<float>();
  run_pins();
  run_pad_pins();
  if (g_findings > 200) printf("... %d findings in all\n", g_findings);
  return g_findings ? 1 : 0;
}
