// vw_api_denoise.cpp -- the denoising entry points of the C ABI: noise sigma, thresholding, transposes, the SWT and
// WaveletDenoiser compositions, and the statistics of the streaming denoiser.
#include "vw_host.h"

using namespace vw;

// ------------------------------------------------------------------------------------------------
// SWT denoise: fused forward -> per-signal exact median of |d_1| -> inverse with fused threshold.
extern "C" vw_status vw_noise_sigma_f64(vw_ctx* c, const double* coeffs, int64_t B, int64_t N, unsigned flags,
                                        double* sigma) {
  if (!c || !coeffs || !sigma) return fail(VW_ERR_NULL, "null argument");
  if (B <= 0 || N <= 0) return fail(VW_ERR_EMPTY, "empty input");
  Staging s(c, flags);
  VW_TRY(s.open());
  VW_TRY(s.in(&coeffs, (size_t)B * N));
  VW_TRY(s.out(&sigma, (size_t)B));
  hipError_t e = launch_noise_sigma(coeffs, N, B, (int)N, 0.0, sigma, nullptr, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return s.finish();
}

extern "C" vw_status vw_threshold_f64(vw_ctx* c, double* coeffs, int64_t B, int64_t N, const double* thr, int soft,
                                      unsigned flags) {
  if (!c || !coeffs || !thr) return fail(VW_ERR_NULL, "null argument");
  if (B <= 0 || N <= 0) return fail(VW_ERR_EMPTY, "empty input");
  Staging s(c, flags);
  VW_TRY(s.open());
  VW_TRY(s.inout(&coeffs, (size_t)B * N));
  VW_TRY(s.in(&thr, (size_t)B));
  hipError_t e = launch_threshold<double>(coeffs, B, N, thr, soft, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return s.finish();
}

// out[c][r] = in[r][c] (rows x cols).  AoS [B][N] -> SoA [N][B] is (rows=B, cols=N); back is
// (rows=N, cols=B).  BatchSIMDMODWT.convertToSoA / convertFromSoA (BatchSIMDMODWT.java:282-308).
template <typename T>
static vw_status transpose_impl(vw_ctx* c, const T* in, int64_t rows, int64_t cols, unsigned flags, T* out) {
  if (!c || !in || !out) return fail(VW_ERR_NULL, "null argument");
  if (rows <= 0 || cols <= 0) return fail(VW_ERR_EMPTY, "empty input");
  if (in == out) return fail(VW_ERR_ARG, "transpose is out of place");
  if ((rows + 63) / 64 > 65535) return fail(VW_ERR_ARG, "rows %lld too large", (long long)rows);
  Staging s(c, flags);
  VW_TRY(s.open());
  const size_t n = (size_t)rows * (size_t)cols;
  VW_TRY(s.in(&in, n));
  VW_TRY(s.out(&out, n));
  hipError_t e;
  {
    LaunchTimer lt(c, "transpose");
    e = launch_transpose<T>(in, rows, cols, out, c->stream);
  }
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return s.finish();
}

extern "C" vw_status vw_transpose_f64(vw_ctx* c, const double* in, int64_t rows, int64_t cols, unsigned flags,
                                      double* out) {
  return transpose_impl<double>(c, in, rows, cols, flags, out);
}

extern "C" vw_status vw_transpose_f32(vw_ctx* c, const float* in, int64_t rows, int64_t cols, unsigned flags,
                                      float* out) {
  return transpose_impl<float>(c, in, rows, cols, flags, out);
}

// B copies of a caller's fixed threshold at thr (device); synchronizes, so not while capturing
static vw_status fixed_threshold(vw_ctx* c, double value, int64_t B, double* thr) {
  if (c->capturing) return fail(VW_ERR_STATE, "a fixed threshold cannot be captured");
  std::vector<double> h((size_t)B, value);
  hipError_t e = hipMemcpyAsync(thr, h.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "threshold stage failed: %s", hipGetErrorString(e));
  return VW_OK;
}

// device pointers; fk: the forward of the call (details / approx unset: they live in the workspace)
static vw_status denoise_device(vw_ctx* c, FwdCall<double> fk, int wid, double threshold, int soft, double* y,
                                double* thr_out) {
  const int64_t B = fk.B, N = fk.N;
  const size_t plane = (size_t)B * (size_t)N;
  // workspace: details [J][B][N] | approx [B][N] | thr [B]   (tiled levels use ws beyond, via a 2nd alloc)
  const size_t coef_bytes = align_up(((size_t)fk.J + 1) * plane * sizeof(double), 256);
  VW_TRY(ensure_ws2(c, coef_bytes + align_up((size_t)B * 8, 256)));
  fk.details = reinterpret_cast<double*>(c->ws2);
  fk.approx = fk.details + (size_t)fk.J * plane;
  double* thr = reinterpret_cast<double*>(reinterpret_cast<char*>(c->ws2) + coef_bytes);
  VW_TRY(forward_impl<double>(c, fk));
  if (threshold < 0) {
    // T = sigma * Math.sqrt(2 * Math.log(n))  core/swt/VectorWaveSwtAdapter.java:514
    const double scale_c = std::sqrt(2 * std::log((double)N));
    LaunchTimer lt(c, "sigma");
    hipError_t e = launch_noise_sigma(fk.details, N, B, (int)N, scale_c, nullptr, thr, c->stream);
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "threshold stage failed: %s", hipGetErrorString(e));
  } else {
    VW_TRY(fixed_threshold(c, threshold, B, thr));
  }
  InvCall<double> ik = inverse_of(fk, y, wid);
  ik.thr = thr; ik.soft = soft;
  VW_TRY(inverse_impl<double>(c, ik));
  if (thr_out && hipMemcpyAsync(thr_out, thr, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
    return fail(VW_ERR_DEVICE, "copy failed");
  return VW_OK;
}

extern "C" vw_status vw_swt_denoise_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                        const double* lo, const double* hi, int L, int wid, int boundary, int J,
                                        double threshold, int soft, unsigned flags, double* y,
                                        double* thresholds_out) {
  VW_TRY(check_common(c, x, y, lo, hi, B, N, L, boundary));
  if (ldx < N) return fail(VW_ERR_ARG, "ldx < N");
  VW_TRY(check_levels(N, L, J, flags));
  if (upsampled_length(L, J) > N && boundary != VW_PERIODIC)
    return fail(VW_ERR_TOO_LARGE, "Upsampled reconstruction filter length exceeds signal length");
  FwdCall<double> k = fwd_call<double>(x, B, N, ldx, lo, hi, L, boundary, J, flags, nullptr, nullptr);
  Staging s(c, flags);
  VW_TRY(s.open());
  VW_TRY(s.in_rows(&k.x, B, N, ldx));
  VW_TRY(s.out(&y, (size_t)B * N));
  VW_TRY(s.out(&thresholds_out, (size_t)B));
  k.flags = s.flags();
  VW_TRY(denoise_device(c, k, wid, threshold, soft, y, thresholds_out));
  return s.finish();
}

// ------------------------------------------------------------------------------------------------
// WaveletDenoiser (core/denoising/WaveletDenoiser.java): forward (single-level MODWTTransform for
// denoise()/denoiseFixed(), MultiLevelMODWTTransform for denoiseMultiLevel()), sigma = MAD of d_1,
// one threshold per (level, signal) by the method (vw_sigma.h), inverse with the per-level threshold
// fused into the detail staging.
// device pointers; fk: the forward of the call, single_level for denoise() / denoiseFixed() (details / approx unset:
// they live in the workspace)
static vw_status wavelet_denoise_device(vw_ctx* c, FwdCall<double> fk, int wid, int method, double fixed, int soft,
                                        double* y, double* thr_out) {
  const int64_t B = fk.B, N = fk.N;
  const int J = fk.J;
  const bool multi = !fk.single_level;
  const size_t plane = (size_t)B * (size_t)N;
  const size_t coef_bytes = align_up(((size_t)J + 1) * plane * sizeof(double), 256);
  VW_TRY(ensure_ws2(c, coef_bytes + align_up((size_t)B * 8, 256) + align_up((size_t)J * B * 8, 256)));
  fk.details = reinterpret_cast<double*>(c->ws2);
  fk.approx = fk.details + (size_t)J * plane;
  double* sig = reinterpret_cast<double*>(reinterpret_cast<char*>(c->ws2) + coef_bytes);
  double* thr = reinterpret_cast<double*>(reinterpret_cast<char*>(sig) + align_up((size_t)B * 8, 256));
  const unsigned fl = fk.flags;
  if (!multi) fk.flags &= ~(unsigned)VW_FLAG_FFT_SWITCH;
  VW_TRY(forward_impl<double>(c, fk));
  if (method == kThrFixed) {
    VW_TRY(fixed_threshold(c, fixed, B, thr));
  } else {
    DenoiseConsts k;
    memset(&k, 0, sizeof(k));
    for (int j = 1; j <= J; ++j) k.level_scale[j - 1] = multi ? std::sqrt((double)(1 << j)) : 1.0;
    k.univ_c = std::sqrt(2.0 * std::log((double)N));
    k.log_n = std::log((double)N);
    k.method = method;
    k.n = (int)N;
    hipError_t e;
    {
      LaunchTimer lt(c, "sigma");
      e = launch_noise_sigma(fk.details, N, B, (int)N, 0.0, sig, nullptr, c->stream);
    }
    if (e == hipSuccess) {
      LaunchTimer lt(c, "threshold");
      e = launch_level_threshold(fk.details, (long long)plane, sig, k, B, J, thr, c->stream);
    }
    if (e != hipSuccess) return fail(VW_ERR_DEVICE, "threshold stage failed: %s", hipGetErrorString(e));
  }
  InvCall<double> ik = inverse_of(fk, y, multi ? wid : VW_WID_OTHER);
  ik.flags = fl; ik.thr = thr; ik.soft = soft;
  if (multi) ik.thr_ld = B;
  VW_TRY(inverse_impl<double>(c, ik));
  if (thr_out && hipMemcpyAsync(thr_out, thr, (size_t)J * B * sizeof(double), hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
    return fail(VW_ERR_DEVICE, "copy failed");
  return VW_OK;
}

extern "C" vw_status vw_wavelet_denoise_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, int64_t ldx,
                                            const double* lo, const double* hi, int L, int wid, int boundary,
                                            int levels, int method, double fixed_threshold, int soft, unsigned flags,
                                            double* y, double* thresholds_out) {
  VW_TRY(check_common(c, x, y, lo, hi, B, N, L, boundary));
  if (ldx < N) return fail(VW_ERR_ARG, "ldx < N");
  if (method < kThrUniversal || method > kThrFixed) return fail(VW_ERR_ARG, "Unknown threshold selection method");
  if (levels < 0) return fail(VW_ERR_LEVEL, "Invalid number of decomposition levels: %d", levels);
  if (levels > 0) {
    // calculateThreshold (:415-424): FIXED needs an explicit threshold (denoiseFixed is single-level)
    if (method == kThrFixed) return fail(VW_ERR_ARG, "Fixed threshold method requires explicit threshold value");
    VW_TRY(check_levels(N, L, levels, flags));
    if (upsampled_length(L, levels) > N && boundary != VW_PERIODIC)
      return fail(VW_ERR_TOO_LARGE, "Upsampled reconstruction filter length exceeds signal length");
  }
  if (method == kThrSure && N > kSureMaxN)
    return fail(VW_ERR_UNSUPPORTED, "SURE threshold on device supports N <= %d (got %lld)", kSureMaxN, (long long)N);
  const int J = levels > 0 ? levels : 1;
  FwdCall<double> k = fwd_call<double>(x, B, N, ldx, lo, hi, L, boundary, J, flags, nullptr, nullptr);
  k.single_level = levels <= 0;
  Staging s(c, flags);
  VW_TRY(s.open());
  VW_TRY(s.in_rows(&k.x, B, N, ldx));
  VW_TRY(s.out(&y, (size_t)B * N));
  VW_TRY(s.out(&thresholds_out, (size_t)J * B));
  k.flags = s.flags();
  VW_TRY(wavelet_denoise_device(c, k, wid, method, fixed_threshold, soft, y, thresholds_out));
  return s.finish();
}

// ------------------------------------------------------------------------------------------------
// Statistics of MODWTStreamingDenoiser (core/modwt/streaming/MODWTStreamingDenoiser.java:133-272):
// MathUtils.median / medianAbsoluteDeviation / standardDeviation on device rows, and the noise-window
// ring update.  Device pointers only (the window lives on the device between blocks).
extern "C" vw_status vw_median_f64(vw_ctx* c, const double* x, int64_t B, int64_t N, const double* center,
                                   unsigned flags, double* median_out) {
  if (!c || !x || !median_out) return fail(VW_ERR_NULL, "null argument");
  if (B <= 0 || N <= 0) return fail(VW_ERR_EMPTY, "Array cannot be null or empty");
  if (N > (1LL << 30)) return fail(VW_ERR_ARG, "row too long");
  if (flags & VW_FLAG_HOST_MEMORY) return fail(VW_ERR_UNSUPPORTED, "device pointers only");
  Staging s(c, flags);
  VW_TRY(s.open());
  hipError_t e;
  if (center && N > kSigmaRegN) {
    // rows beyond the register-keyed centered path: deviations |x - center| into their own scratch (not ws: growing ws
    // invalidates graphs that never ran a median), then the uncentered selection (any N) on them -- the same keys, the
    // same exact order statistic
    if (B > 65535) return fail(VW_ERR_UNSUPPORTED, "centered median of more than 65535 long rows");
    VW_TRY(grow_buffer(c, &c->med, &c->med_bytes, (size_t)B * (size_t)N * sizeof(double), 0, "median scratch"));
    double* dev = reinterpret_cast<double*>(c->med);
    e = launch_abs_center(x, N, B, (int)N, center, dev, c->stream);
    if (e == hipSuccess) e = launch_median(dev, N, B, (int)N, nullptr, median_out, c->stream);
  } else {
    e = launch_median(x, N, B, (int)N, center, median_out, c->stream);
  }
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return s.finish();
}

extern "C" vw_status vw_stddev_f64(vw_ctx* c, const double* x, int64_t N, unsigned flags, double* out) {
  if (!c || !x || !out) return fail(VW_ERR_NULL, "null argument");
  if (N < 2) return fail(VW_ERR_ARG, "Need at least 2 values for standard deviation");
  if (N > (1LL << 30)) return fail(VW_ERR_ARG, "too many values");
  if (flags & VW_FLAG_HOST_MEMORY) return fail(VW_ERR_UNSUPPORTED, "device pointers only");
  Staging s(c, flags);
  VW_TRY(s.open());
  hipError_t e = launch_seq_std(x, (int)N, out, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return s.finish();
}

// window[(start + k) % wsize] = |src[idx[k]]| for k < count; idx is a HOST array (the stratified
// sampling positions are integer bookkeeping, computed by the caller), staged to the device here.
extern "C" vw_status vw_window_gather_abs_f64(vw_ctx* c, const double* src, const int32_t* idx, int64_t count,
                                              double* window, int64_t wsize, int64_t start) {
  if (!c || !src || !window || (count > 0 && !idx)) return fail(VW_ERR_NULL, "null argument");
  if (wsize <= 0 || count < 0 || count > wsize || start < 0 || start >= wsize) return fail(VW_ERR_ARG, "bad window");
  if (count == 0) return ok();
  Staging s(c, 0);
  if (c->capturing) return fail(VW_ERR_STATE, "cannot be captured");
  const int32_t* di = nullptr;
  VW_TRY(s.upload(idx, (size_t)count, &di));
  hipError_t e = launch_gather_abs(src, di, (int)count, window, (int)wsize, (int)start, c->stream);
  if (e != hipSuccess) return fail(VW_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return s.finish();  // (synchronizes: the index copy's bytes are the next call's)
}
