// vw_api_modwt.cpp -- the transform entry points of the C ABI: multi-level forward / inverse (equal-length and
// two-length banks), the round trip, the multi-context forms, the single-level transform and streaming blocks.
#include "vw_host.h"

#include <thread>

using namespace vw;

// ------------------------------------------------------------------------------------------------
// Forward / inverse of B rows, arguments checked.  Host memory: details are J host planes `det_stride` elements
// apart (B * N for a whole batch; the global B * N for a row block of a sharded batch).
template <typename T>
static vw_status forward_staged(vw_ctx* c, FwdCall<T> k, int64_t det_stride) {
  Staging s(c, k.flags);
  VW_TRY(s.open());
  const size_t plane = (size_t)(k.B * k.N);
  VW_TRY(s.in_rows(&k.x, k.B, k.N, k.ldx));
  VW_TRY(s.out_planes(&k.details, (size_t)k.J, plane, (size_t)det_stride));
  VW_TRY(s.out(&k.approx, plane));
  k.flags = s.flags();
  VW_TRY(forward_impl<T>(c, k));
  return s.finish();
}

template <typename T>
static vw_status inverse_staged(vw_ctx* c, InvCall<T> k, int64_t det_stride) {
  Staging s(c, k.flags);
  VW_TRY(s.open());
  const size_t plane = (size_t)(k.B * k.N);
  // planes the call does not read are not staged (and no host address reaches the planner)
  if (s.host() && !k.detail_mask) k.details = nullptr;
  if (s.host() && k.approx_zero) k.approx = nullptr;
  VW_TRY(s.in_planes(&k.details, (size_t)k.J, plane, (size_t)det_stride));
  VW_TRY(s.in(&k.approx, plane));
  VW_TRY(s.out(&k.y, plane));
  k.flags = s.flags();
  VW_TRY(inverse_impl<T>(c, k));
  return s.finish();
}

template <typename T>
static vw_status modwt_forward(vw_ctx* c, const FwdCall<T>& k) {
  VW_TRY(check_forward(c, k, k.details, k.approx));
  return forward_staged(c, k, k.B * k.N);
}

template <typename T>
static vw_status modwt_inverse(vw_ctx* c, const InvCall<T>& k) {
  VW_TRY(check_inverse(c, k));
  return inverse_staged(c, k, k.B * k.N);
}

template <typename T>
static InvCall<T> masked(InvCall<T> k, unsigned detail_mask, int approx_zero) {
  k.detail_mask = detail_mask;
  k.approx_zero = approx_zero;
  return k;
}

extern "C" vw_status vw_modwt_forward_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                          const double* lo, const double* hi, int L, int wid, int boundary, int J,
                                          unsigned flags, double* details, double* approx) {
  (void)wid;
  return modwt_forward(c, fwd_call(x, B, N, ldx, lo, hi, L, boundary, J, flags, details, approx));
}
extern "C" vw_status vw_modwt_forward_f32(vw_ctx* c, const float* x, int64_t B, int64_t N, int64_t ldx,
                                          const double* lo, const double* hi, int L, int wid, int boundary, int J,
                                          unsigned flags, float* details, float* approx) {
  (void)wid;
  return modwt_forward(c, fwd_call(x, B, N, ldx, lo, hi, L, boundary, J, flags, details, approx));
}
extern "C" vw_status vw_modwt_inverse_f64(vw_ctx* c, const double* details, const double* approx, int64_t B,
                                          int64_t N, const double* lo, const double* hi, int L, int wid, int boundary,
                                          int J, unsigned detail_mask, int approx_zero, unsigned flags, double* y) {
  return modwt_inverse(c, masked(inv_call(details, approx, B, N, lo, hi, L, wid, boundary, J, flags, y), detail_mask,
                                 approx_zero));
}
extern "C" vw_status vw_modwt_inverse_f32(vw_ctx* c, const float* details, const float* approx, int64_t B,
                                          int64_t N, const double* lo, const double* hi, int L, int wid, int boundary,
                                          int J, unsigned detail_mask, int approx_zero, unsigned flags, float* y) {
  return modwt_inverse(c, masked(inv_call(details, approx, B, N, lo, hi, L, wid, boundary, J, flags, y), detail_mask,
                                 approx_zero));
}

// ------------------------------------------------------------------------------------------------
// Forward, then inverse of its coefficients (include/vectorwave_amd.h): one k_roundtrip launch where the pair is
// eligible (pair_fusable) and the launch shape is, or can be made, ready; the two calls otherwise.

// The one launch; *done stays false, with nothing queued, where the pair takes the two calls.
static vw_status roundtrip_fused(vw_ctx* c, FwdCall<double> fk, InvCall<double> ik, bool* done) {
  Staging s(c, fk.flags);
  if (!c->tune.pair_fuse || check_levels(fk.N, fk.L, fk.J, fk.flags) != VW_OK || s.open() != VW_OK ||
      capture_guard(c, fk.flags) != VW_OK)
    return VW_OK;
  fk.cus = ik.cus = c->cus;
  FwdPlan<double> fp;
  InvPlan<double> ip;
  plan_forward(c->tune, fk, &fp);
  plan_inverse(c->tune, ik, &ip);
  PairLaunch l;
  if (!(pair_fusable(fk, fp, ik, ip) &&
        (c->capturing ||
         pair_prepare(fp.args.taps, fp.fma, fp.threads, fp.lds, c->tune.pair_keep, nullptr, nullptr) == hipSuccess) &&
        pair_launch_shape(fp.args.taps, fp.fma, fp.threads, fp.lds, c->tune.pair_keep, fk.B, c->cus, &l))) {
    (void)hipGetLastError();
    return VW_OK;
  }
  *done = true;
  FwdArgs<double> f = fp.args;
  f.x = fk.x; f.details = fk.details; f.approx = fk.approx;
  f.bad = c->bad;
  copy_bank(f.lo, f.hi, fk, f.taps, f.taps_hi);
  PairArgs<double> a;
  pair_args(f, ik, ip, &a);
  {
    LaunchTimer lt(c, "roundtrip");
    hipError_t e = launch_roundtrip(a, l, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "round-trip launch failed: %s", hipGetErrorString(e));
  }
  return s.finish();
}

extern "C" vw_status vw_modwt_roundtrip_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                            const double* lo, const double* hi, const double* rlo, const double* rhi,
                                            int L, int wid, int boundary, int J, unsigned flags, double* details,
                                            double* approx, double* y) {
  const FwdCall<double> fk = fwd_call(x, B, N, ldx, lo, hi, L, boundary, J, flags, details, approx);
  InvCall<double> ik = inverse_of(fk, y, wid);
  ik.lo = rlo; ik.hi = rhi;
  if (c && x && details && approx && y && lo && hi && rlo && rhi && !(flags & VW_FLAG_HOST_MEMORY) && B > 0 && N > 0 &&
      ldx >= N && L >= 1 && L <= kPairMaxTaps && J >= 1 && J <= kMaxLevels && boundary == VW_PERIODIC) {
    bool done = false;
    const vw_status st = roundtrip_fused(c, fk, ik, &done);
    if (done) return st;
  }
  // the two calls, with their own argument checks
  VW_TRY(modwt_forward(c, fk));
  return modwt_inverse(c, ik);
}

// The round-trip launch for rows of N samples on this context: the variant VW_PAIR_KEEP and the occupancies choose
// (kept detail planes) and its resident workgroups per CU; both 0 where the shape is not eligible.
static vw_status roundtrip_variant(vw_ctx* c, int64_t N, int L, int J, unsigned flags, int* keep, int* per_cu) {
  *keep = *per_cu = 0;
  if (N <= 0 || N > (1LL << 30) || L < 1 || L > kPairMaxTaps || J < 1 || J > kMaxLevels) return ok();
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (c->capturing) return fail(VW_ERR_STATE, "occupancy queries cannot be captured");
  hipSetDevice(c->device);
  // the planner reads a pointer's alignment and nothing behind it
  double* const aligned = reinterpret_cast<double*>(uintptr_t(4096));
  static const double taps[kPairMaxTaps] = {0};
  FwdCall<double> fk = fwd_call<double>(aligned, 4LL * c->cus, N, N, taps, taps, L, VW_PERIODIC, J, flags & VW_FLAG_FMA,
                                        aligned, aligned);
  fk.cus = c->cus;
  FwdPlan<double> fp;
  plan_forward(c->tune, fk, &fp);
  if (fp.error != VW_OK || !pair_forward_shape(fp)) return ok();
  if (pair_prepare(fp.args.taps, fp.fma, fp.threads, fp.lds, c->tune.pair_keep, per_cu, keep) != hipSuccess) {
    (void)hipGetLastError();
    *keep = *per_cu = 0;
  }
  return ok();
}

extern "C" vw_status vw_roundtrip_occupancy(vw_ctx* c, int64_t N, int L, int J, unsigned flags, int* per_cu) {
  if (!c || !per_cu) return fail(VW_ERR_NULL, "null argument");
  int keep;
  return roundtrip_variant(c, N, L, J, flags, &keep, per_cu);
}

extern "C" vw_status vw_roundtrip_variant(vw_ctx* c, int64_t N, int L, int J, unsigned flags, int* keep, int* per_cu) {
  if (!c || !keep || !per_cu) return fail(VW_ERR_NULL, "null argument");
  return roundtrip_variant(c, N, L, J, flags, keep, per_cu);
}

// ------------------------------------------------------------------------------------------------
// Biorthogonal banks (BiorthogonalSpline / ReverseBiorthogonalSpline): lo has Llo taps, hi has Lhi.  Equal
// lengths are the calls above, argument for argument.
static int bank_hi(int Llo, int Lhi) { return Lhi == Llo ? 0 : Lhi; }
static vw_status bank_arg(int Lhi) {
  if (Lhi < 1 || Lhi > kMaxTaps) return fail(VW_ERR_ARG, "filter length %d unsupported (1..%d)", Lhi, kMaxTaps);
  return VW_OK;
}
extern "C" vw_status vw_modwt_forward_bi_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                             const double* lo, int Llo, const double* hi, int Lhi, int wid,
                                             int boundary, int J, unsigned flags, double* details, double* approx) {
  (void)wid;
  VW_TRY(bank_arg(Lhi));
  return modwt_forward(c, fwd_call(x, B, N, ldx, lo, hi, Llo, boundary, J, flags, details, approx, bank_hi(Llo, Lhi)));
}
extern "C" vw_status vw_modwt_forward_bi_f32(vw_ctx* c, const float* x, int64_t B, int64_t N, int64_t ldx,
                                             const double* lo, int Llo, const double* hi, int Lhi, int wid,
                                             int boundary, int J, unsigned flags, float* details, float* approx) {
  (void)wid;
  VW_TRY(bank_arg(Lhi));
  return modwt_forward(c, fwd_call(x, B, N, ldx, lo, hi, Llo, boundary, J, flags, details, approx, bank_hi(Llo, Lhi)));
}
extern "C" vw_status vw_modwt_inverse_bi_f64(vw_ctx* c, const double* details, const double* approx, int64_t B,
                                             int64_t N, const double* lo, int Llo, const double* hi, int Lhi, int wid,
                                             int boundary, int J, unsigned detail_mask, int approx_zero,
                                             unsigned flags, double* y) {
  VW_TRY(bank_arg(Lhi));
  return modwt_inverse(c, masked(inv_call(details, approx, B, N, lo, hi, Llo, wid, boundary, J, flags, y,
                                          bank_hi(Llo, Lhi)), detail_mask, approx_zero));
}
extern "C" vw_status vw_modwt_inverse_bi_f32(vw_ctx* c, const float* details, const float* approx, int64_t B,
                                             int64_t N, const double* lo, int Llo, const double* hi, int Lhi, int wid,
                                             int boundary, int J, unsigned detail_mask, int approx_zero,
                                             unsigned flags, float* y) {
  VW_TRY(bank_arg(Lhi));
  return modwt_inverse(c, masked(inv_call(details, approx, B, N, lo, hi, Llo, wid, boundary, J, flags, y,
                                          bank_hi(Llo, Lhi)), detail_mask, approx_zero));
}

// ------------------------------------------------------------------------------------------------
// One batch over several contexts, one host thread per context ("each device has its
// own context, stream, input generator and output buffers; one host thread per device").  The
// reference parallelises one call in-process too (VectorWaveSwtAdapter.java:210-267 executor,
// BatchMODWT.multiLevelAoS :90-111 over a batch); here the batch is split into contiguous row
// blocks (vectorwave_amd/shard.py shard_rows: the first B % n blocks get one extra row) and block k
// runs on ctxs[k] from its own std::thread -- no exchange between devices.  Host memory only (the
// JNI / FFM caller's arrays): each thread stages its block through its context.
static void shard_block(int64_t B, int n, int k, int64_t* start, int64_t* rows) {
  const int64_t base = B / n, extra = B % n;
  *start = k * base + std::min<int64_t>(k, extra);
  *rows = base + (k < extra ? 1 : 0);
}

static vw_status check_ctxs(vw_ctx* const* ctxs, int nctx) {
  if (!ctxs) return fail(VW_ERR_NULL, "ctxs is null");
  if (nctx < 1) return fail(VW_ERR_ARG, "need at least one context (got %d)", nctx);
  for (int k = 0; k < nctx; ++k)
    if (!ctxs[k]) return fail(VW_ERR_NULL, "ctxs[%d] is null", k);
  return VW_OK;
}

// fn(k) for k < n, one host thread each (k = 0 on the calling thread); the first failing k's status, its message
// behind label(k).
template <typename F, typename G>
static vw_status run_threads(int n, F&& fn, G&& label) {
  struct Res { vw_status st = VW_OK; std::string msg; int64_t idx = -1; };
  std::vector<Res> res(n);
  auto work = [&](int k) {
    const vw_status st = fn(k);
    res[k].st = st;
    if (st != VW_OK) { res[k].msg = err_state().msg; res[k].idx = err_state().index; }
  };
  std::vector<std::thread> th;
  th.reserve(n);
  for (int k = 1; k < n; ++k) th.emplace_back(work, k);
  work(0);
  for (auto& t : th) t.join();
  for (int k = 0; k < n; ++k)
    if (res[k].st != VW_OK) {
      err_state().msg = label(k) + ": " + res[k].msg;
      err_state().index = res[k].idx;
      return res[k].st;
    }
  return ok();
}

// fn(k) on context k
template <typename F>
static vw_status run_per_ctx(vw_ctx* const* ctxs, int nctx, F&& fn) {
  VW_TRY(check_ctxs(ctxs, nctx));
  return run_threads(nctx, fn, [](int k) { return "context " + std::to_string(k); });
}

// fn(context, first row, rows) on each row block of the batch
template <typename F>
static vw_status run_sharded(vw_ctx* const* ctxs, int nctx, int64_t B, F&& fn) {
  VW_TRY(check_ctxs(ctxs, nctx));
  if (B <= 0) return fail(VW_ERR_EMPTY, "batch must be non-empty (B=%lld)", (long long)B);
  const int used = (int)std::min<int64_t>(nctx, B);
  return run_threads(
      used,
      [&](int k) {
        int64_t start, rows;
        shard_block(B, used, k, &start, &rows);
        err_state().signal_base = start;  // signal numbers in this thread's error messages count from row 0 of the batch
        const vw_status st = fn(ctxs[k], start, rows);
        err_state().signal_base = 0;
        return st;
      },
      [&](int k) {
        int64_t start, rows;
        shard_block(B, used, k, &start, &rows);
        return "block " + std::to_string(k) + " (rows " + std::to_string(start) + ".." +
               std::to_string(start + rows - 1) + ")";
      });
}

extern "C" vw_status vw_modwt_forward_multi_f64(vw_ctx* const* ctxs, int nctx, const double* x, int64_t B, int64_t N,
                                                int64_t ldx, const double* lo, const double* hi, int L, int wid,
                                                int boundary, int J, unsigned flags, double* details,
                                                double* approx) {
  (void)wid;
  if (!(flags & VW_FLAG_HOST_MEMORY)) return fail(VW_ERR_ARG, "multi-context calls take host memory (VW_FLAG_HOST_MEMORY)");
  if (!x || !details || !approx || !lo || !hi) return fail(VW_ERR_NULL, "null array argument");
  if (ldx < N) return fail(VW_ERR_ARG, "ldx (%lld) < N (%lld)", (long long)ldx, (long long)N);
  const FwdCall<double> k = fwd_call(x, B, N, ldx, lo, hi, L, boundary, J, flags, details, approx);
  return run_sharded(ctxs, nctx, B, [&](vw_ctx* c, int64_t start, int64_t rows) -> vw_status {
    FwdCall<double> kb = k;  // the block's rows of every array
    kb.x += start * ldx; kb.details += start * N; kb.approx += start * N; kb.B = rows;
    VW_TRY(check_common(c, kb.x, kb.details, lo, hi, rows, N, L, boundary));
    VW_TRY(check_levels(N, L, J, flags));
    return forward_staged(c, kb, B * N);
  });
}

extern "C" vw_status vw_modwt_inverse_multi_f64(vw_ctx* const* ctxs, int nctx, const double* details,
                                                const double* approx, int64_t B, int64_t N, const double* lo,
                                                const double* hi, int L, int wid, int boundary, int J,
                                                unsigned detail_mask, int approx_zero, unsigned flags, double* y) {
  if (!(flags & VW_FLAG_HOST_MEMORY)) return fail(VW_ERR_ARG, "multi-context calls take host memory (VW_FLAG_HOST_MEMORY)");
  if (!y || !lo || !hi) return fail(VW_ERR_NULL, "null argument");
  if (!details && detail_mask) return fail(VW_ERR_NULL, "details is null");
  if (!approx && !approx_zero) return fail(VW_ERR_NULL, "approx is null");
  VW_TRY(check_inverse_levels(N, L, J, flags));
  const InvCall<double> k =
      masked(inv_call(details, approx, B, N, lo, hi, L, wid, boundary, J, flags, y), detail_mask, approx_zero);
  return run_sharded(ctxs, nctx, B, [&](vw_ctx* c, int64_t start, int64_t rows) -> vw_status {
    InvCall<double> kb = k;  // the block's rows of every array
    if (details) kb.details += start * N;
    if (approx) kb.approx += start * N;
    kb.y += start * N; kb.B = rows;
    VW_TRY(check_common(c, kb.y, kb.y, lo, hi, rows, N, L, boundary));
    return inverse_staged(c, kb, B * N);
  });
}

extern "C" vw_status vw_modwt_forward_multi_dev_f64(vw_ctx* const* ctxs, int nctx, const double* const* x,
                                                    const int64_t* rows, int64_t N, int64_t ldx, const double* lo,
                                                    const double* hi, int L, int wid, int boundary, int J,
                                                    unsigned flags, double* const* details,
                                                    double* const* approx) {
  (void)wid;
  if (flags & VW_FLAG_HOST_MEMORY)
    return fail(VW_ERR_ARG, "device-resident multi-context calls take device memory (no VW_FLAG_HOST_MEMORY)");
  if (!x || !rows || !details || !approx) return fail(VW_ERR_NULL, "null array argument");
  return run_per_ctx(ctxs, nctx, [&](int k) -> vw_status {
    if (rows[k] == 0) return VW_OK;
    return modwt_forward(ctxs[k], fwd_call(x[k], rows[k], N, ldx, lo, hi, L, boundary, J, flags, details[k], approx[k]));
  });
}

extern "C" vw_status vw_modwt_inverse_multi_dev_f64(vw_ctx* const* ctxs, int nctx, const double* const* details,
                                                    const double* const* approx, const int64_t* rows, int64_t N,
                                                    const double* lo, const double* hi, int L, int wid,
                                                    int boundary, int J, unsigned detail_mask, int approx_zero,
                                                    unsigned flags, double* const* y) {
  if (flags & VW_FLAG_HOST_MEMORY)
    return fail(VW_ERR_ARG, "device-resident multi-context calls take device memory (no VW_FLAG_HOST_MEMORY)");
  if (!rows || !y || (!details && detail_mask) || (!approx && !approx_zero))
    return fail(VW_ERR_NULL, "null array argument");
  return run_per_ctx(ctxs, nctx, [&](int k) -> vw_status {
    if (rows[k] == 0) return VW_OK;
    return modwt_inverse(ctxs[k], masked(inv_call<double>(details ? details[k] : nullptr, approx ? approx[k] : nullptr,
                                                          rows[k], N, lo, hi, L, wid, boundary, J, flags, y[k]),
                                         detail_mask, approx_zero));
  });
}

// ------------------------------------------------------------------------------------------------
// Single level (MODWTTransform): any N >= 1 (no L <= N guard), pairwise inverse sums.
// k.Lhi: the high-pass length of a two-length bank (0 = L)
static vw_status modwt1_forward(vw_ctx* c, FwdCall<double> k) {
  VW_TRY(check_common(c, k.x, k.details, k.lo, k.hi, k.B, k.N, k.L, k.boundary));
  if (!k.approx) return fail(VW_ERR_NULL, "approx is null");
  if (k.ldx < k.N) return fail(VW_ERR_ARG, "ldx < N");
  Staging s(c, k.flags);
  VW_TRY(s.open());
  const size_t plane = (size_t)(k.B * k.N);
  VW_TRY(s.in_rows(&k.x, k.B, k.N, k.ldx));
  VW_TRY(s.out(&k.approx, plane));
  VW_TRY(s.out(&k.details, plane));
  if ((k.flags & VW_FLAG_BATCH_HAAR) && k.L == 2 && k.Lhi == 0 && k.boundary == VW_PERIODIC) {  // the batch path's Haar
    LaunchTimer lt(c, "forward1");
    hipError_t e = launch_single_haar_batch<double>(k.x, k.ldx, k.B, (int)k.N, k.approx, k.details, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  } else {
    k.flags = s.flags() & ~VW_FLAG_FFT_SWITCH;
    k.single_level = true;
    VW_TRY(forward_impl<double>(c, k));
  }
  return s.finish();
}

extern "C" vw_status vw_modwt1_forward_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                           const double* lo, const double* hi, int L, int boundary, unsigned flags,
                                           double* approx, double* detail) {
  return modwt1_forward(c, fwd_call(x, B, N, ldx, lo, hi, L, boundary, 1, flags, detail, approx));
}
extern "C" vw_status vw_modwt1_forward_bi_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                              const double* lo, int Llo, const double* hi, int Lhi, int boundary,
                                              unsigned flags, double* approx, double* detail) {
  VW_TRY(bank_arg(Lhi));
  return modwt1_forward(c, fwd_call(x, B, N, ldx, lo, hi, Llo, boundary, 1, flags, detail, approx, bank_hi(Llo, Lhi)));
}

static vw_status modwt1_inverse(vw_ctx* c, InvCall<double> k) {
  VW_TRY(check_common(c, k.approx, k.details, k.lo, k.hi, k.B, k.N, k.L, k.boundary));
  if (!k.y) return fail(VW_ERR_NULL, "y is null");
  Staging s(c, k.flags);
  VW_TRY(s.open());
  const size_t plane = (size_t)(k.B * k.N);
  VW_TRY(s.in(&k.approx, plane));
  VW_TRY(s.in(&k.details, plane));
  VW_TRY(s.out(&k.y, plane));
  k.flags = s.flags();
  k.detail_mask = 1u;
  k.single_level = true;
  VW_TRY(inverse_impl<double>(c, k));
  return s.finish();
}

extern "C" vw_status vw_modwt1_inverse_f64(vw_ctx* c, const double* approx, const double* detail, int64_t B,
                                           int64_t N, const double* lo, const double* hi, int L, int boundary,
                                           unsigned flags, double* y) {
  return modwt1_inverse(c, inv_call(detail, approx, B, N, lo, hi, L, VW_WID_OTHER, boundary, 1, flags, y));
}
extern "C" vw_status vw_modwt1_inverse_bi_f64(vw_ctx* c, const double* approx, const double* detail, int64_t B,
                                              int64_t N, const double* lo, int Llo, const double* hi, int Lhi,
                                              int boundary, unsigned flags, double* y) {
  VW_TRY(bank_arg(Lhi));
  return modwt1_inverse(c, inv_call(detail, approx, B, N, lo, hi, Llo, VW_WID_OTHER, boundary, 1, flags, y,
                                    bank_hi(Llo, Lhi)));
}

// ------------------------------------------------------------------------------------------------
// Streaming (BatchStreamingMODWT)
extern "C" vw_status vw_stream_create(vw_ctx* c, const double* lo, const double* hi, int L, int boundary, int levels,
                                      vw_stream** out) {
  if (!c || !lo || !hi || !out) return fail(VW_ERR_NULL, "null argument");
  if (levels < 1) return fail(VW_ERR_ARG, "levels must be >= 1");
  if (levels > kMaxLevels) return fail(VW_ERR_ARG, "levels too large");
  if (L < 1 || L > kMaxTaps) return fail(VW_ERR_ARG, "bad filter length");
  if (boundary < VW_PERIODIC || boundary > VW_ZERO_PADDING) return fail(VW_ERR_BOUNDARY, "bad boundary");
  vw_stream* s = new vw_stream();
  s->ctx = c;
  s->lo.assign(lo, lo + L);
  s->hi.assign(hi, hi + L);
  s->L = L;
  s->boundary = boundary;
  s->levels = levels;
  s->hist.assign(levels, nullptr);
  s->snap.assign(levels, nullptr);
  s->hist_len.resize(levels);
  for (int j = 1; j <= levels; ++j) s->hist_len[j - 1] = (int)(upsampled_length(L, j) - 1);
  *out = s;
  return ok();
}

static void free_hist(vw_stream* s) {
  for (auto* v : {&s->hist, &s->snap})
    for (auto& p : *v) {
      if (p) hipFree(p);
      p = nullptr;
    }
}

extern "C" vw_status vw_stream_destroy(vw_stream* s) {
  if (!s) return fail(VW_ERR_NULL, "stream is null");
  hipSetDevice(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  free_hist(s);
  delete s;
  return ok();
}

extern "C" int64_t vw_stream_batch(vw_stream* s) { return s ? s->last_batch : -1; }

extern "C" int64_t vw_stream_history_length(vw_stream* s, int level) {
  if (!s || level < 1 || level > s->levels) return -1;
  return s->hist_len[level - 1];
}

// a block (or the flush tail) of n samples per row through the stream's filters and levels
static FwdCall<double> stream_call(vw_stream* s, const double* blk, int64_t B, int64_t n, unsigned flags,
                                   double* details, double* approx) {
  return fwd_call(blk, B, n, n, s->lo.data(), s->hi.data(), s->L, s->boundary, s->levels, flags, details, approx);
}

// device pointers; PERIODIC blocks are whole transforms (processMultiLevel PERIODIC -> BatchMODWT.multiLevelAoS, no
// cap, BatchStreamingMODWT.java:115-116), the others read, and unless flushing leave, the level histories
static vw_status stream_run(vw_stream* s, FwdCall<double> k, bool flush) {
  if (s->boundary != VW_PERIODIC) {
    const bool first = !s->hist_init;
    k.mode_override = first ? -1 : kHaloHistory;
    k.hist = s->hist.data();
    k.hist_update = !flush;
    k.hist_snap = !flush && s->snap[0] ? s->snap.data() : nullptr;
    k.hist_first = first;
  }
  return forward_impl<double>(s->ctx, k);
}

extern "C" vw_status vw_stream_process_f64(vw_stream* s, const double* block, int64_t B, int64_t n, unsigned flags,
                                           double* details, double* approx) {
  if (!s) return fail(VW_ERR_NULL, "stream is null");
  vw_ctx* c = s->ctx;
  FwdCall<double> k = stream_call(s, block, B, n, flags, details, approx);
  VW_TRY(check_common(c, k.x, k.details, k.lo, k.hi, B, n, k.L, k.boundary));
  if (!approx) return fail(VW_ERR_NULL, "approx is null");
  Staging sg(c, flags);
  VW_TRY(sg.open());
  if (s->boundary != VW_PERIODIC) {
    // ensureHistoryCapacity  BatchStreamingMODWT.java:310-324: batch change re-initialises history
    if (s->last_batch != B) {
      free_hist(s);
      for (int j = 0; j < s->levels; ++j)
        VW_HIP(hipMalloc(&s->hist[j], std::max<size_t>((size_t)B * s->hist_len[j] * sizeof(double), 16)));
      s->hist_init = false;
      s->last_batch = B;
    }
    if ((flags & VW_FLAG_REF_NONFINITE) && !s->snap[0])
      for (int j = 0; j < s->levels; ++j)
        VW_HIP(hipMalloc(&s->snap[j], std::max<size_t>((size_t)B * s->hist_len[j] * sizeof(double), 16)));
  }
  const size_t plane = (size_t)(B * n);
  VW_TRY(sg.in(&k.x, plane));
  VW_TRY(sg.out(&k.details, (size_t)s->levels * plane));
  VW_TRY(sg.out(&k.approx, plane));
  k.flags = sg.flags();
  VW_TRY(stream_run(s, k, false));
  VW_TRY(sg.finish());
  if (s->boundary != VW_PERIODIC) s->hist_init = true;
  return ok();
}

// flushMultiLevel  BatchStreamingMODWT.java:231-275: tail from level-1 history (ZERO: zeros;
// SYMMETRIC: hist[histLen-1-t]), run through every level's history without updating it.
extern "C" vw_status vw_stream_flush_f64(vw_stream* s, int64_t tail_len, unsigned flags, double* details,
                                         double* approx) {
  if (!s) return fail(VW_ERR_NULL, "stream is null");
  vw_ctx* c = s->ctx;
  if (s->boundary == VW_PERIODIC) return fail(VW_ERR_UNSUPPORTED, "Flush is only applicable to ZERO_PADDING/SYMMETRIC");
  if (tail_len <= 0) return ok();
  if (!s->hist_init || s->last_batch <= 0) return fail(VW_ERR_STATE, "No prior blocks processed; cannot flush");
  int min_hist = s->hist_len[0];
  for (int j = 0; j < s->levels; ++j) min_hist = std::min(min_hist, s->hist_len[j]);
  if (tail_len > min_hist)
    return fail(VW_ERR_ARG, "tailLength (%lld) exceeds maximum allowed across levels (%d)", (long long)tail_len,
                min_hist);
  if (!details || !approx) return fail(VW_ERR_NULL, "null output");
  Staging sg(c, flags);
  if (c->capturing) return fail(VW_ERR_STATE, "flush cannot be captured");
  const int64_t B = s->last_batch;
  const int h0 = s->hist_len[0];
  std::vector<double> hist((size_t)B * h0), tail((size_t)B * tail_len, 0.0);
  if (s->boundary == VW_SYMMETRIC) {
    VW_HIP(hipMemcpyAsync(hist.data(), s->hist[0], hist.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    VW_HIP(hipStreamSynchronize(c->stream));
    for (int64_t b = 0; b < B; ++b)
      for (int64_t t = 0; t < tail_len; ++t) tail[b * tail_len + t] = hist[b * h0 + (h0 - 1 - t)];
  }
  FwdCall<double> k = stream_call(s, nullptr, B, tail_len, sg.flags(), details, approx);
  VW_TRY(sg.upload(tail.data(), tail.size(), &k.x));  // the tail is this call's own: staged on device-pointer calls too
  VW_TRY(sg.out(&k.details, (size_t)s->levels * B * tail_len));
  VW_TRY(sg.out(&k.approx, (size_t)B * tail_len));
  VW_TRY(stream_run(s, k, true));
  return sg.finish();
}
