// vw_api_analysis.cpp -- the analysis entry points of the C ABI: financial metrics, wavelet energy per level,
// multiresolution analysis, the continuous wavelet transform and its inverse.
#include "vw_host.h"

using namespace vw;

// ------------------------------------------------------------------------------------------------
// com.morphiqlabs.financial (vw_fin.hip): FinancialAnalyzer's four metrics and FinancialWaveletAnalyzer's
// Sharpe ratios, one workgroup per row, one launch per call (the non-periodic wavelet Sharpe composes the
// single-level forward and inverse in ws2 first).

static vw_status fin_common(vw_ctx* c, const void* in, const void* out, int64_t B, unsigned flags) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  if (!in || !out) return fail(VW_ERR_NULL, "null array argument");
  if (B <= 0) return fail(VW_ERR_EMPTY, "batch must be non-empty (B=%lld)", (long long)B);
  if (flags & VW_FLAG_FMA)
    return fail(VW_ERR_ARG, "VW_FLAG_FMA is not supported by the financial calls (fused taps change the detail signs)");
  return VW_OK;
}

static vw_status fin_taps(const double* lo, const double* hi, int L, FinArgs* a) {
  if (!lo || !hi) return fail(VW_ERR_NULL, "null filter argument");
  if (L < 1 || L > kFinMaxTaps) return fail(VW_ERR_ARG, "filter length %d unsupported (1..%d)", L, kFinMaxTaps);
  const double s = 1.0 / std::sqrt(2.0);  // as copy_taps
  for (int i = 0; i < kFinMaxTaps; ++i) {
    a->lo[i] = i < L ? lo[i] * s : 0.0;
    a->hi[i] = i < L ? hi[i] * s : 0.0;
  }
  a->L = L;
  return VW_OK;
}

// the kernel's validation word -> status.  Bit 62: a return that overflowed between two finite prices
// (the reference's transform.forward rejects it); clear: a non-finite input element.
static vw_status fin_report(unsigned long long bad, int64_t N, bool prices) {
  if (bad == ~0ull) return VW_OK;
  const bool overflow = (bad >> 62) & 1ull;
  const unsigned long long flat = bad & ((1ull << 62) - 1);
  const long long i = (long long)(flat % (unsigned long long)N);
  const long long b = (long long)(flat / (unsigned long long)N) + (long long)err_state().signal_base;
  vw_status st;
  if (prices && !overflow)
    st = fail(VW_ERR_ARG, "Prices must contain only finite values (index %lld, signal %lld)", i, b);
  else
    st = fail(VW_ERR_NONFINITE, "%s contains non-finite value at index %lld (signal %lld)",
              prices ? "returns" : "signal", i, b);
  err_state().index = (int64_t)(b * (long long)N + i);
  return st;
}

// the rows, flags and workspace words every financial call sets
static void fin_shape(vw_ctx* c, FinArgs* a, int64_t B, int64_t N, int64_t ld, unsigned flags) {
  a->B = B; a->N = (int)N; a->ld = ld;
  a->tree = (flags & VW_FLAG_TREE_SUMS) ? 1 : 0;
  a->bad = c->bad;
}

static vw_status fin_launch(vw_ctx* c, const FinArgs& a, bool analyze) {
  if (a.validate) VW_HIP(hipMemsetAsync(c->bad, 0xFF, sizeof(unsigned long long), c->stream));
  {
    LaunchTimer lt(c, "fin");
    hipError_t e = analyze ? launch_fin_analyze(a, c->stream) : launch_fin_sharpe(a, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  }
  if (a.validate) {
    unsigned long long bad = ~0ull;
    VW_TRY(read_bad(c, &bad));
    VW_TRY(fin_report(bad, a.N, analyze));
  }
  return VW_OK;
}

extern "C" vw_status vw_fin_analyze_f64(vw_ctx* c, const double* prices, int64_t B, int64_t N, int64_t ld,
                                        const double* lo, const double* hi, int L, double anomaly_k, unsigned flags,
                                        double* out) {
  VW_TRY(fin_common(c, prices, out, B, flags));
  FinArgs a{};
  VW_TRY(fin_taps(lo, hi, L, &a));
  if (N < 2) return fail(VW_ERR_ARG, "Prices must contain at least 2 elements");
  if (ld < N) return fail(VW_ERR_ARG, "ld (%lld) < N (%lld)", (long long)ld, (long long)N);
  if (N - 1 > kFinMaxN)
    return fail(VW_ERR_UNSUPPORTED, "financial analysis keeps a row's coefficients in LDS: at most %d returns per row",
                kFinMaxN);
  Staging s(c, flags);
  VW_TRY(s.open());
  VW_TRY(capture_guard(c, flags));
  fin_shape(c, &a, B, N, ld, flags);
  a.k = anomaly_k;
  a.validate = (flags & VW_FLAG_VALIDATE) ? 1 : 0;
  a.x = prices; a.out = out;
  VW_TRY(s.in_rows(&a.x, B, N, ld));
  VW_TRY(s.out(&a.out, (size_t)5 * B));
  VW_TRY(fin_launch(c, a, true));
  return s.finish();
}

static const char* const kSingleReturnMsg =
    "Cannot calculate Sharpe ratio with a single return value. "
    "At least 2 returns are required to calculate standard deviation (risk).";

static vw_status fin_sharpe_checks(int64_t N, int64_t ld) {
  if (N <= 0) return fail(VW_ERR_EMPTY, "Returns array cannot be empty");
  if (N == 1) return fail(VW_ERR_ARG, "%s", kSingleReturnMsg);
  if (ld < N) return fail(VW_ERR_ARG, "ld (%lld) < N (%lld)", (long long)ld, (long long)N);
  if (N > kFinMaxN)
    return fail(VW_ERR_UNSUPPORTED, "the Sharpe calls keep a row in LDS: at most %d returns per row", kFinMaxN);
  return VW_OK;
}

extern "C" vw_status vw_fin_sharpe_f64(vw_ctx* c, const double* returns, int64_t B, int64_t N, int64_t ld,
                                       double risk_free, unsigned flags, double* out) {
  VW_TRY(fin_common(c, returns, out, B, flags));
  VW_TRY(fin_sharpe_checks(N, ld));
  Staging s(c, flags);
  VW_TRY(s.open());
  VW_TRY(capture_guard(c, flags));
  FinArgs a{};
  fin_shape(c, &a, B, N, ld, flags);  // (the reference's plain Sharpe ratio does not validate: VW_FLAG_VALIDATE checks nothing here)
  a.k = risk_free;
  a.x = returns; a.out = out;
  VW_TRY(s.in_rows(&a.x, B, N, ld));
  VW_TRY(s.out(&a.out, (size_t)B));
  VW_TRY(fin_launch(c, a, false));
  return s.finish();
}

// device pointers in, device pointer out
static vw_status wavelet_sharpe_device(vw_ctx* c, FinArgs a, const double* lo, const double* hi, int boundary,
                                       unsigned flags) {
  if (boundary == VW_PERIODIC) {
    a.wavelet = 1;
    a.validate = (flags & VW_FLAG_VALIDATE) ? 1 : 0;
    return fin_launch(c, a, false);
  }
  // ZERO_PADDING / SYMMETRIC: the existing single-level kernels, planes approx | detail | y in ws2
  const size_t plane = (size_t)a.B * (size_t)a.N;
  VW_TRY(ensure_ws2(c, 3 * plane * sizeof(double)));
  double* da = reinterpret_cast<double*>(c->ws2);
  double* dd = da + plane;
  double* dy = dd + plane;
  FwdCall<double> fk = fwd_call(a.x, (int64_t)a.B, (int64_t)a.N, (int64_t)a.ld, lo, hi, a.L, boundary, 1,
                                flags & (VW_FLAG_VALIDATE | VW_FLAG_REF_NONFINITE), dd, da);
  fk.single_level = true;
  VW_TRY(forward_impl<double>(c, fk));
  VW_HIP(hipMemsetAsync(dd, 0, plane * sizeof(double), c->stream));  // `new double[detailCoeffs.length]`
  InvCall<double> ik = inverse_of(fk, dy);
  ik.flags = fk.flags & ~VW_FLAG_VALIDATE;
  VW_TRY(inverse_impl<double>(c, ik));
  a.x = dy;
  a.ld = a.N;
  return fin_launch(c, a, false);
}

extern "C" vw_status vw_fin_wavelet_sharpe_f64(vw_ctx* c, const double* returns, int64_t B, int64_t N, int64_t ld,
                                               const double* lo, const double* hi, int L, int boundary,
                                               double risk_free, unsigned flags, double* out) {
  VW_TRY(fin_common(c, returns, out, B, flags));
  FinArgs a{};
  VW_TRY(fin_taps(lo, hi, L, &a));
  if (boundary < VW_PERIODIC || boundary > VW_ZERO_PADDING)
    return fail(VW_ERR_BOUNDARY, "MODWT only supports PERIODIC, ZERO_PADDING, and SYMMETRIC boundary modes");
  VW_TRY(fin_sharpe_checks(N, ld));
  Staging s(c, flags);
  VW_TRY(s.open());
  VW_TRY(capture_guard(c, flags));
  fin_shape(c, &a, B, N, ld, flags);
  a.k = risk_free;
  a.x = returns; a.out = out;
  VW_TRY(s.in_rows(&a.x, B, N, ld));
  VW_TRY(s.out(&a.out, (size_t)B));
  VW_TRY(wavelet_sharpe_device(c, a, lo, hi, boundary, s.flags()));
  return s.finish();
}

// ------------------------------------------------------------------------------------------------
// Wavelet energy per level (vw_energy.hip): MultiLevelMODWTResultImpl.getApproximationEnergy /
// getDetailEnergyAtLevel (:91-117, computeEnergy :211-216) per signal, out [J+1][B].
// Timing families: "energy_fused" (k_energy_fused), "energy_chain" (sequential plane sums), "energy_tree".

// device pointers in, device pointer out
static vw_status energy_planes_device(vw_ctx* c, const double* details, const double* approx, int64_t B, int64_t N,
                                      int J, unsigned flags, double* out) {
  EnergyPlanesArgs a{};
  a.approx = approx; a.details = details; a.B = B; a.N = (int)N; a.J = J; a.out = out;
  a.vec_io = (N % 2 == 0) && ((uintptr_t)approx & 15u) == 0 && ((uintptr_t)details & 15u) == 0;
  const bool tree = flags & VW_FLAG_TREE_SUMS;
  LaunchTimer lt(c, tree ? "energy_tree" : "energy_chain");
  hipError_t e = launch_energy_planes(a, tree, c->cus, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "energy launch failed: %s", hipGetErrorString(e));
  return VW_OK;
}

// device pointers in, device pointer out; arguments checked by the caller.  fk: the forward whose coefficients are
// summed (its details / approx are set here where they are materialised)
static vw_status energy_device(vw_ctx* c, FwdCall<double> fk, double* out) {
  VW_TRY(capture_guard(c, fk.flags));
  fk.cus = c->cus;
  EnergyPlan p;
  plan_energy(c->tune, fk, &p);
  if (p.fused) {
    EnergyArgs a = p.args;
    a.x = fk.x; a.out = out;
    copy_taps(a.lo, fk.lo, fk.L);
    copy_taps(a.hi, fk.hi, fk.L);
    LaunchTimer lt(c, "energy_fused");
    hipError_t e = launch_energy_fused(a, p.threads, p.lds, p.fma, p.nv, p.grid, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "energy launch failed: %s", hipGetErrorString(e));
    return VW_OK;
  }
  // the forward's own plan and executor into the workspace (approx [B][N] | details [J][B][N]), then the plane sums
  const size_t plane = (size_t)fk.B * (size_t)fk.N;
  VW_TRY(ensure_ws2(c, ((size_t)fk.J + 1) * plane * sizeof(double)));
  fk.approx = reinterpret_cast<double*>(c->ws2);
  fk.details = fk.approx + plane;
  VW_TRY(forward_impl<double>(c, fk));
  return energy_planes_device(c, fk.details, fk.approx, fk.B, fk.N, fk.J, fk.flags, out);
}

extern "C" vw_status vw_modwt_energy_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                         const double* lo, const double* hi, int L, int wid, int boundary, int J,
                                         unsigned flags, double* out) {
  (void)wid;
  FwdCall<double> k = fwd_call<double>(x, B, N, ldx, lo, hi, L, boundary, J, flags, nullptr, nullptr);
  VW_TRY(check_forward(c, k, out, out));
  Staging s(c, flags);
  VW_TRY(s.open());
  VW_TRY(s.in_rows(&k.x, B, N, ldx));
  VW_TRY(s.out(&out, ((size_t)J + 1) * B));
  k.flags = s.flags();
  VW_TRY(energy_device(c, k, out));
  return s.finish();
}

extern "C" vw_status vw_energy_planes_f64(vw_ctx* c, const double* details, const double* approx, int64_t B,
                                          int64_t N, int J, unsigned flags, double* out) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  if (!approx || !out || (!details && J > 0)) return fail(VW_ERR_NULL, "null array argument");
  if (B <= 0) return fail(VW_ERR_EMPTY, "batch must be non-empty (B=%lld)", (long long)B);
  if (N <= 0) return fail(VW_ERR_EMPTY, "Signal cannot be empty");
  if (N > (1LL << 30)) return fail(VW_ERR_ARG, "signal length %lld too large", (long long)N);
  if (J < 0 || J > kMaxLevels) return fail(VW_ERR_LEVEL, "levels must be in 0..%d", kMaxLevels);
  if (flags & ~(unsigned)(VW_FLAG_TREE_SUMS | VW_FLAG_HOST_MEMORY | VW_FLAG_SYNC))
    return fail(VW_ERR_ARG, "vw_energy_planes_f64 takes TREE_SUMS, HOST_MEMORY and SYNC only");
  Staging s(c, flags);
  VW_TRY(s.open());
  const size_t plane = (size_t)B * (size_t)N;
  if (s.host() && J == 0) details = nullptr;  // (not read)
  VW_TRY(s.in(&approx, plane));
  VW_TRY(s.in(&details, (size_t)J * plane));
  VW_TRY(s.out(&out, ((size_t)J + 1) * B));
  VW_TRY(energy_planes_device(c, details, approx, B, N, J, flags, out));
  return s.finish();
}

// ------------------------------------------------------------------------------------------------
// Multiresolution analysis (vw_mra.hip): out[c] = the inverse with detail_mask = c ? 1 << (c-1) : 0 and
// approx_zero = (c != 0) (VectorWaveSwtAdapter.extractLevel :576-598), every c in one call.
// Timing families: "mra" (k_mra); the loop path's launches count as "inverse" / "inverse_level".

// device pointers; k.y = out [J+1][B][N]; arguments checked by the caller
template <typename T>
static vw_status mra_planes_device(vw_ctx* c, InvCall<T> k) {
  VW_TRY(capture_guard(c, k.flags));
  k.cus = c->cus;
  MraPlan<T> p;
  plan_mra(c->tune, k, &p);
  if (p.fused) {
    MraArgs<T> a = p.args;
    a.details = k.details; a.approx = k.approx; a.out = k.y;
    copy_taps(a.lo, k.lo, k.L);
    copy_taps(a.hi, k.hi, k.L);
    LaunchTimer lt(c, "mra");
    hipError_t e = launch_mra<T>(a, p.threads, p.lds, p.fma, p.nv, p.grid, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "mra launch failed: %s", hipGetErrorString(e));
    return VW_OK;
  }
  // the loop path: the J+1 masked inverses, each through its own plan
  const size_t plane = (size_t)k.B * (size_t)k.N;
  for (int comp = 0; comp <= k.J; ++comp) {
    InvCall<T> ik = k;
    ik.detail_mask = comp ? 1u << (comp - 1) : 0u;
    ik.approx_zero = comp != 0;
    ik.y = k.y + (size_t)comp * plane;
    VW_TRY(inverse_impl<T>(c, ik));
  }
  return VW_OK;
}

template <typename T>
static vw_status mra_planes(vw_ctx* c, InvCall<T> k) {
  VW_TRY(check_inverse(c, k));
  if (k.flags & ~(unsigned)(VW_FLAG_CORE_LEVELS | VW_FLAG_FMA | VW_FLAG_HOST_MEMORY | VW_FLAG_SYNC | VW_FLAG_VALIDATE |
                            VW_FLAG_REF_NONFINITE))
    return fail(VW_ERR_ARG, "vw_mra_planes takes CORE_LEVELS, FMA, HOST_MEMORY, SYNC, VALIDATE and REF_NONFINITE only");
  Staging s(c, k.flags);
  VW_TRY(s.open());
  const size_t plane = (size_t)k.B * (size_t)k.N;
  VW_TRY(s.in(&k.details, (size_t)k.J * plane));
  VW_TRY(s.in(&k.approx, plane));
  VW_TRY(s.out(&k.y, ((size_t)k.J + 1) * plane));
  k.flags = s.flags();
  VW_TRY(mra_planes_device<T>(c, k));
  return s.finish();
}

// device pointers; the forward's own plan and executor into the workspace (approx [B][N] | details [J][B][N]), then
// the planes call on those coefficients
template <typename T>
static vw_status mra_device(vw_ctx* c, FwdCall<T> fk, int wid, T* out) {
  VW_TRY(capture_guard(c, fk.flags));
  const size_t plane = (size_t)fk.B * (size_t)fk.N;
  VW_TRY(ensure_ws2(c, ((size_t)fk.J + 1) * plane * sizeof(T)));
  fk.approx = reinterpret_cast<T*>(c->ws2);
  fk.details = fk.approx + plane;
  VW_TRY(forward_impl<T>(c, fk));
  InvCall<T> ik = inverse_of(fk, out, wid);
  ik.flags = fk.flags & ~(unsigned)VW_FLAG_FFT_SWITCH;
  return mra_planes_device<T>(c, ik);
}

// fk: the forward of the call (details / approx unset: they live in the workspace)
template <typename T>
static vw_status modwt_mra(vw_ctx* c, FwdCall<T> fk, int wid, T* out) {
  // vw_modwt_forward_*'s checks, in its order, then those of the inverse that the forward's have not made
  VW_TRY(check_forward(c, fk, out, out));
  VW_TRY(check_inverse_levels(fk.N, fk.L, fk.J, fk.flags));
  if (fk.flags & ~(unsigned)(VW_FLAG_CORE_LEVELS | VW_FLAG_FMA | VW_FLAG_HOST_MEMORY | VW_FLAG_SYNC | VW_FLAG_VALIDATE |
                             VW_FLAG_REF_NONFINITE | VW_FLAG_FFT_SWITCH))
    return fail(VW_ERR_ARG, "vw_modwt_mra takes CORE_LEVELS, FFT_SWITCH, FMA, HOST_MEMORY, SYNC, VALIDATE and REF_NONFINITE only");
  Staging s(c, fk.flags);
  VW_TRY(s.open());
  VW_TRY(s.in_rows(&fk.x, fk.B, fk.N, fk.ldx));
  VW_TRY(s.out(&out, ((size_t)fk.J + 1) * (size_t)fk.B * (size_t)fk.N));
  fk.flags = s.flags();
  VW_TRY(mra_device<T>(c, fk, wid, out));
  return s.finish();
}

extern "C" vw_status vw_mra_planes_f64(vw_ctx* c, const double* details, const double* approx, int64_t B, int64_t N,
                                       const double* lo, const double* hi, int L, int wid, int boundary, int J,
                                       unsigned flags, double* out) {
  return mra_planes(c, inv_call(details, approx, B, N, lo, hi, L, wid, boundary, J, flags, out));
}
extern "C" vw_status vw_mra_planes_f32(vw_ctx* c, const float* details, const float* approx, int64_t B, int64_t N,
                                       const double* lo, const double* hi, int L, int wid, int boundary, int J,
                                       unsigned flags, float* out) {
  return mra_planes(c, inv_call(details, approx, B, N, lo, hi, L, wid, boundary, J, flags, out));
}
extern "C" vw_status vw_modwt_mra_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx, const double* lo,
                                      const double* hi, int L, int wid, int boundary, int J, unsigned flags,
                                      double* out) {
  return modwt_mra(c, fwd_call<double>(x, B, N, ldx, lo, hi, L, boundary, J, flags, nullptr, nullptr), wid, out);
}
extern "C" vw_status vw_modwt_mra_f32(vw_ctx* c, const float* x, int64_t B, int64_t N, int64_t ldx, const double* lo,
                                      const double* hi, int L, int wid, int boundary, int J, unsigned flags,
                                      float* out) {
  return modwt_mra(c, fwd_call<float>(x, B, N, ldx, lo, hi, L, boundary, J, flags, nullptr, nullptr), wid, out);
}

// ------------------------------------------------------------------------------------------------
// Continuous wavelet transform (vw_cwt.hip): fixed-order correlations of each row with one table per scale, plan_cwt's
// launches heaviest scales first.  Timing family: "cwt".

// A call's table image `img` (its first `bytes` go to the device) into a slot of the context: *dev of *dev_bytes,
// *resident the host image it holds.  The same image again uploads nothing.  A new one bumps ws_gen (graphs
// recorded on the old tables are stale) and cannot be recorded.
static vw_status image_upload(vw_ctx* c, void** dev, size_t* dev_bytes, std::vector<unsigned char>* resident,
                              std::vector<unsigned char>* img, size_t bytes, const char* who) {
  if (*img == *resident) return VW_OK;
  if (c->capturing)
    return fail(VW_ERR_STATE, "%s: new tables cannot be uploaded during a capture (run the call once first)", who);
  if (*dev_bytes < bytes) {
    VW_HIP(hipStreamSynchronize(c->stream));
    if (*dev) hipFree(*dev);
    *dev = nullptr; *dev_bytes = 0; resident->clear();
    VW_HIP(hipMalloc(dev, bytes));
    *dev_bytes = bytes;
  }
  resident->clear();  // (not valid until the copy is enqueued)
  VW_HIP(hipMemcpyAsync(*dev, img->data(), bytes, hipMemcpyHostToDevice, c->stream));
  VW_HIP(hipStreamSynchronize(c->stream));  // img is this call's
  resident->swap(*img);
  ++c->ws_gen;
  return VW_OK;
}

// The call's device image: [CwtScaleDev x S, plan order][taps_re x ntaps][taps_im x ntaps], T-typed, 16-byte aligned
// parts.  Kept in the context: the same image again uploads nothing.  A new one bumps ws_gen (graphs recorded on
// the old tables are stale) and cannot be recorded.
template <typename T>
static vw_status cwt_upload(vw_ctx* c, const CwtPlan& p, const vw_cwt_scale* scales, int S, const double* taps_re,
                            const double* taps_im, int64_t ntaps, CwtArgs<T>* a) {
  const size_t sc_bytes = align_up((size_t)S * sizeof(CwtScaleDev<T>), 16);
  const size_t tab_bytes = align_up((size_t)ntaps * sizeof(T), 16);
  const size_t bytes = sc_bytes + tab_bytes * (taps_im ? 2 : 1);
  std::vector<unsigned char> img(bytes + 2, 0);
  img[bytes] = (unsigned char)sizeof(T);  // the layout's own parameters close the image
  img[bytes + 1] = taps_im ? 1 : 0;
  CwtScaleDev<T>* hs = reinterpret_cast<CwtScaleDev<T>*>(img.data());
  for (int i = 0; i < S; ++i) {
    const vw_cwt_scale& d = scales[p.order[i].scale];
    CwtScaleDev<T> e;
    std::memset(&e, 0, sizeof(e));  // the image is compared byte for byte, padding included
    e.tap_begin = (int)d.tap_begin; e.taps = d.taps; e.window = d.window_begin; e.scale = p.order[i].scale;
    e.divisor = (T)d.divisor;
    std::memcpy(&hs[i], &e, sizeof(e));
  }
  T* hre = reinterpret_cast<T*>(img.data() + sc_bytes);
  for (int64_t i = 0; i < ntaps; ++i) hre[i] = (T)taps_re[i];
  if (taps_im) {
    T* him = reinterpret_cast<T*>(img.data() + sc_bytes + tab_bytes);
    for (int64_t i = 0; i < ntaps; ++i) him[i] = (T)taps_im[i];
  }
  VW_TRY(image_upload(c, &c->cwt_dev, &c->cwt_dev_bytes, &c->cwt_img, &img, bytes, "vw_cwt"));
  const unsigned char* base = static_cast<const unsigned char*>(c->cwt_dev);
  a->sc = reinterpret_cast<const CwtScaleDev<T>*>(base);
  a->taps_re = reinterpret_cast<const T*>(base + sc_bytes);
  a->taps_im = taps_im ? reinterpret_cast<const T*>(base + sc_bytes + tab_bytes) : nullptr;
  return VW_OK;
}

template <typename T>
static vw_status cwt_impl(vw_ctx* c, const T* x, int64_t B, int64_t N, int64_t ldx, const vw_cwt_scale* scales, int S,
                          const double* taps_re, const double* taps_im, int64_t ntaps, int ext, int64_t wrap,
                          unsigned flags, T* out_re, T* out_im) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  if (!x || !scales || !taps_re || !out_re || (taps_im && !out_im)) return fail(VW_ERR_NULL, "null array argument");
  if (B <= 0) return fail(VW_ERR_EMPTY, "batch must be non-empty (B=%lld)", (long long)B);
  if (N <= 0) return fail(VW_ERR_EMPTY, "Signal cannot be empty");
  if (S <= 0) return fail(VW_ERR_EMPTY, "Scales cannot be empty");
  if (N > (1LL << 30)) return fail(VW_ERR_ARG, "signal length %lld too large", (long long)N);
  if (ldx < N) return fail(VW_ERR_ARG, "ldx (%lld) < N (%lld)", (long long)ldx, (long long)N);
  if (flags & ~(unsigned)(VW_FLAG_FMA | VW_FLAG_HOST_MEMORY | VW_FLAG_SYNC))
    return fail(VW_ERR_ARG, "vw_cwt takes FMA, HOST_MEMORY and SYNC only");
  if (ext < VW_CWT_ZERO || ext > VW_CWT_WRAP_ZERO) return fail(VW_ERR_ARG, "unknown extension %d", ext);
  if (ext == VW_CWT_WRAP_ZERO && wrap < 1) return fail(VW_ERR_ARG, "VW_CWT_WRAP_ZERO needs wrap >= 1 (wrap=%lld)", (long long)wrap);
  if (ntaps < 1 || ntaps > (1LL << 30)) return fail(VW_ERR_ARG, "ntaps (%lld) outside 1..2^30", (long long)ntaps);
  std::vector<int> K((size_t)S);
  for (int s = 0; s < S; ++s) {
    const vw_cwt_scale& d = scales[s];
    if (d.taps < 1) return fail(VW_ERR_ARG, "scale %d has %d taps", s, (int)d.taps);
    if (d.tap_begin < 0 || d.tap_begin > ntaps - d.taps)
      return fail(VW_ERR_ARG, "scale %d reads taps [%lld, %lld) outside the table of %lld", s, (long long)d.tap_begin,
                  (long long)d.tap_begin + d.taps, (long long)ntaps);
    if (!(d.divisor > 0.0) || !((T)d.divisor > (T)0) || std::isinf((T)d.divisor))
      return fail(VW_ERR_ARG, "scale %d has divisor %g (must be positive and finite)", s, d.divisor);
    if (d.window_begin > (1 << 30) || d.window_begin < -(1 << 30))
      return fail(VW_ERR_ARG, "scale %d has window_begin %d outside +-2^30", s, (int)d.window_begin);
    K[s] = d.taps;
  }
  CwtCall k;
  k.B = B; k.N = N; k.S = S; k.taps = K.data(); k.elem_bytes = (int)sizeof(T); k.cplx = taps_im != nullptr; k.ext = ext;
  k.flags = flags;
  CwtPlan p;
  plan_cwt(k, &p);
  if (p.error != VW_OK) return fail((vw_status)p.error, "%s", p.msg);

  Staging stg(c, flags);
  VW_TRY(stg.open());
  CwtArgs<T> a{};
  VW_TRY(cwt_upload<T>(c, p, scales, S, taps_re, taps_im, ntaps, &a));
  const CwtScaleDev<T>* const sc0 = a.sc;
  a.ldx = ldx; a.B = B; a.N = (int)N; a.S = S; a.ntiles = p.ntiles; a.ext = ext; a.wrap = wrap > 0 ? wrap : 1;
  const size_t planes = (size_t)B * (size_t)S * (size_t)N;
  a.x = x; a.out_re = out_re; a.out_im = taps_im ? out_im : nullptr;
  VW_TRY(stg.in_rows(&a.x, B, N, ldx));
  VW_TRY(stg.out(&a.out_re, planes));
  VW_TRY(stg.out(&a.out_im, planes));
  for (const CwtLaunch& l : p.launches) {
    a.sc = sc0 + l.first; a.nsc = l.count;
    LaunchTimer lt(c, "cwt");
    hipError_t e = launch_cwt<T>(a, p.threads, l.lds, p.cplx, p.fma, l.grid, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "cwt launch failed: %s", hipGetErrorString(e));
  }
  return stg.finish();
}

extern "C" vw_status vw_cwt_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx, const vw_cwt_scale* scales,
                                int S, const double* taps_re, const double* taps_im, int64_t ntaps, int ext, int64_t wrap,
                                unsigned flags, double* out_re, double* out_im) {
  return cwt_impl<double>(c, x, B, N, ldx, scales, S, taps_re, taps_im, ntaps, ext, wrap, flags, out_re, out_im);
}
extern "C" vw_status vw_cwt_f32(vw_ctx* c, const float* x, int64_t B, int64_t N, int64_t ldx, const vw_cwt_scale* scales,
                                int S, const double* taps_re, const double* taps_im, int64_t ntaps, int ext, int64_t wrap,
                                unsigned flags, float* out_re, float* out_im) {
  return cwt_impl<float>(c, x, B, N, ldx, scales, S, taps_re, taps_im, ntaps, ext, wrap, flags, out_re, out_im);
}

// ------------------------------------------------------------------------------------------------
// Inverse continuous wavelet transform (vw_icwt.hip): InverseCWT.reconstruct on coefficient planes, plan_icwt's one
// launch (SUM) or one thread per output (DIRECT).  Timing family: "icwt".

// The call's device image: [IcwtScaleDev x nsc, the caller's order][taps x ntaps], T-typed, 16-byte aligned parts,
// in the context's slot of its own (image_upload).
template <typename T>
static vw_status icwt_upload(vw_ctx* c, const vw_icwt_scale* scales, int nsc, const double* taps, int64_t ntaps,
                             IcwtArgs<T>* a) {
  const size_t sc_bytes = align_up((size_t)nsc * sizeof(IcwtScaleDev<T>), 16);
  const size_t tab_bytes = align_up((size_t)ntaps * sizeof(T), 16);
  const size_t bytes = sc_bytes + tab_bytes;
  std::vector<unsigned char> img(bytes + 1, 0);
  img[bytes] = (unsigned char)sizeof(T);  // the layout's own parameter closes the image
  IcwtScaleDev<T>* hs = reinterpret_cast<IcwtScaleDev<T>*>(img.data());
  for (int i = 0; i < nsc; ++i) {
    const vw_icwt_scale& d = scales[i];
    IcwtScaleDev<T> e;
    std::memset(&e, 0, sizeof(e));  // the image is compared byte for byte, padding included
    e.tap_begin = (int)d.tap_begin; e.taps = d.taps; e.window = d.window_begin; e.plane = d.plane;
    e.weight = (T)d.weight; e.scale = (T)d.scale;
    std::memcpy(&hs[i], &e, sizeof(e));
  }
  T* ht = reinterpret_cast<T*>(img.data() + sc_bytes);
  for (int64_t i = 0; i < ntaps; ++i) ht[i] = (T)taps[i];
  VW_TRY(image_upload(c, &c->icwt_dev, &c->icwt_dev_bytes, &c->icwt_img, &img, bytes, "vw_icwt"));
  const unsigned char* base = static_cast<const unsigned char*>(c->icwt_dev);
  a->sc = reinterpret_cast<const IcwtScaleDev<T>*>(base);
  a->taps = reinterpret_cast<const T*>(base + sc_bytes);
  return VW_OK;
}

template <typename T>
static vw_status icwt_impl(vw_ctx* c, const T* coef, int64_t B, int S, int64_t N, int64_t ldc,
                           const vw_icwt_scale* scales, int nsc, const double* taps, int64_t ntaps, int form,
                           int64_t wrap, double divisor, unsigned flags, T* out, int64_t ldo) {
  if (!c) return fail(VW_ERR_NULL, "ctx is null");
  if (!coef || !scales || !taps || !out) return fail(VW_ERR_NULL, "null array argument");
  if (B <= 0) return fail(VW_ERR_EMPTY, "batch must be non-empty (B=%lld)", (long long)B);
  if (N <= 0) return fail(VW_ERR_EMPTY, "Signal cannot be empty");
  if (S <= 0 || nsc <= 0) return fail(VW_ERR_EMPTY, "Scales cannot be empty");
  if (N > (1LL << 30)) return fail(VW_ERR_ARG, "signal length %lld too large", (long long)N);
  if (ldc < N) return fail(VW_ERR_ARG, "ldc (%lld) < N (%lld)", (long long)ldc, (long long)N);
  if (ldo < N) return fail(VW_ERR_ARG, "ldo (%lld) < N (%lld)", (long long)ldo, (long long)N);
  if (flags & ~(unsigned)(VW_FLAG_FMA | VW_FLAG_HOST_MEMORY | VW_FLAG_SYNC))
    return fail(VW_ERR_ARG, "vw_icwt takes FMA, HOST_MEMORY and SYNC only");
  if (form != VW_ICWT_SUM && form != VW_ICWT_DIRECT) return fail(VW_ERR_ARG, "unknown form %d", form);
  if (form == VW_ICWT_DIRECT && (flags & VW_FLAG_FMA))
    return fail(VW_ERR_ARG, "VW_FLAG_FMA is not supported by VW_ICWT_DIRECT (every term ends in a division)");
  if (form == VW_ICWT_SUM && wrap < N)
    return fail(VW_ERR_ARG, "VW_ICWT_SUM needs wrap >= N (wrap=%lld, N=%lld)", (long long)wrap, (long long)N);
  if (!(divisor > 0.0) || !((T)divisor > (T)0) || std::isinf((T)divisor))
    return fail(VW_ERR_ARG, "divisor %g (must be positive and finite)", divisor);
  if (ntaps < 1 || ntaps > (1LL << 30)) return fail(VW_ERR_ARG, "ntaps (%lld) outside 1..2^30", (long long)ntaps);
  std::vector<int> K((size_t)nsc);
  for (int j = 0; j < nsc; ++j) {
    const vw_icwt_scale& d = scales[j];
    if (d.taps < 1) return fail(VW_ERR_ARG, "scale %d has %d taps", j, (int)d.taps);
    if (d.tap_begin < 0 || d.tap_begin > ntaps - d.taps)
      return fail(VW_ERR_ARG, "scale %d reads taps [%lld, %lld) outside the table of %lld", j, (long long)d.tap_begin,
                  (long long)d.tap_begin + d.taps, (long long)ntaps);
    if (d.plane < 0 || d.plane >= S) return fail(VW_ERR_ARG, "scale %d reads plane %d outside [0, %d)", j, (int)d.plane, S);
    if (d.window_begin > (1 << 30) || d.window_begin < -(1 << 30))
      return fail(VW_ERR_ARG, "scale %d has window_begin %d outside +-2^30", j, (int)d.window_begin);
    if (form == VW_ICWT_DIRECT && d.taps != 2 * N - 1)
      return fail(VW_ERR_ARG, "scale %d has %d taps: VW_ICWT_DIRECT reads 2N - 1 = %lld", j, (int)d.taps, (long long)(2 * N - 1));
    K[j] = d.taps;
  }
  IcwtCall k;
  k.B = B; k.N = N; k.nsc = nsc; k.taps = K.data(); k.elem_bytes = (int)sizeof(T); k.flags = flags;
  IcwtPlan p;
  plan_icwt(k, &p);
  if (p.error != VW_OK) return fail((vw_status)p.error, "%s", p.msg);

  Staging stg(c, flags);
  VW_TRY(stg.open());
  IcwtArgs<T> a{};
  VW_TRY(icwt_upload<T>(c, scales, nsc, taps, ntaps, &a));
  a.B = B; a.N = (int)N; a.S = S; a.nsc = nsc; a.ntiles = p.ntiles; a.wrap = form == VW_ICWT_SUM ? wrap : N;
  a.divisor = (T)divisor;
  a.coef = coef; a.ldc = ldc; a.out = out; a.ldo = ldo;
  if (stg.host()) {  // rows packed on the device: the host's padding is neither read nor written
    VW_TRY(stg.in_planes(&a.coef, (size_t)B * (size_t)S, (size_t)N, (size_t)ldc));
    VW_TRY(stg.out_planes(&a.out, (size_t)B, (size_t)N, (size_t)ldo));
    a.ldc = N; a.ldo = N;
  }
  {
    LaunchTimer lt(c, "icwt");
    hipError_t e = form == VW_ICWT_SUM ? launch_icwt<T>(a, p.threads, p.lds, p.fma, p.grid, c->stream)
                                       : launch_icwt_direct<T>(a, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "icwt launch failed: %s", hipGetErrorString(e));
  }
  return stg.finish();
}

extern "C" vw_status vw_icwt_f64(vw_ctx* c, const double* coef, int64_t B, int S, int64_t N, int64_t ldc,
                                 const vw_icwt_scale* scales, int nsc, const double* taps, int64_t ntaps, int form,
                                 int64_t wrap, double divisor, unsigned flags, double* out, int64_t ldo) {
  return icwt_impl<double>(c, coef, B, S, N, ldc, scales, nsc, taps, ntaps, form, wrap, divisor, flags, out, ldo);
}
extern "C" vw_status vw_icwt_f32(vw_ctx* c, const float* coef, int64_t B, int S, int64_t N, int64_t ldc,
                                 const vw_icwt_scale* scales, int nsc, const double* taps, int64_t ntaps, int form,
                                 int64_t wrap, double divisor, unsigned flags, float* out, int64_t ldo) {
  return icwt_impl<float>(c, coef, B, S, N, ldc, scales, nsc, taps, ntaps, form, wrap, divisor, flags, out, ldo);
}
