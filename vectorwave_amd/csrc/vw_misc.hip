// vw_misc.hip -- the small utility kernels (streaming history, threshold, fill, Haar batch, transpose) and the
// launchers of those and of the denoiser's statistics kernels (vw_sigma.h).
#define VW_MISC_UNIT 1
#include "vw_launch_k.h"
#include "vw_dev_core.h"
#include "vw_sigma.h"

namespace vw {

int fused_max_threads() { return kMaxThreads; }

template <typename T>
__global__ void k_history_update(const T* __restrict__ in, long long ld_in, const T* __restrict__ old_hist,
                                 T* __restrict__ new_hist, int n, int hist_len) {
  const long long b = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= hist_len) return;
  const int q = p + n - hist_len;
  new_hist[b * hist_len + p] = q >= 0 ? in[b * ld_in + q] : old_hist[b * hist_len + p + n];
}

template <typename T>
__global__ void k_threshold(T* c, long long B, long long N, const T* __restrict__ thr, int soft) {
  const long long total = B * N;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / N;
    c[i] = threshold_t(c[i], thr[b], soft);
  }
}

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <typename T>
__global__ void k_fill_uniform(T* x, long long count, unsigned long long seed, long long offset) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < count;
       i += (long long)gridDim.x * blockDim.x) {
    const unsigned long long r = splitmix64(seed ^ (unsigned long long)(offset + i));
    const double u = (double)(r >> 11) * (1.0 / 9007199254740992.0);
    x[i] = (T)(2.0 * u - 1.0);
  }
}

// BatchSIMDMODWT.haarBatchMODWTSoA (:86-140): hard-coded 0.5 / -0.5 taps.
template <typename T>
__global__ void k_single_haar_batch(const T* __restrict__ x, long long ldx, int N, T* approx, T* detail) {
  const long long b = blockIdx.y;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < N; t += gridDim.x * blockDim.x) {
    const int tm1 = (t - 1 + N) % N;
    const T s0 = x[b * ldx + t], s1 = x[b * ldx + tm1];
    approx[b * (size_t)N + t] = s0 * T(0.5) + s1 * T(0.5);
    detail[b * (size_t)N + t] = s0 * T(0.5) + s1 * T(-0.5);
  }
}

template <typename T>
hipError_t launch_history_update(const T* in, long long ld_in, const T* old_hist, T* new_hist, long long B, int n,
                                 int hist_len, hipStream_t st) {
  if (hist_len <= 0) return hipSuccess;
  return launch_k<k_history_update<T>>(dim3((unsigned)((hist_len + 255) / 256), (unsigned)B), dim3(256), 0, st, in, ld_in,
                                       old_hist, new_hist, n, hist_len);
}

static hipError_t run_sigma(const double* x, long long ld, long long B, int N, double scale_c, double* sigma_out,
                            double* thr_out, const double* center, double* median_out, hipStream_t st) {
  return launch_k<k_noise_sigma>(dim3((unsigned)B), dim3(kSigmaThreads), 0, st, x, ld, N, scale_c, sigma_out, thr_out,
                                 center, median_out);
}

hipError_t launch_noise_sigma(const double* coeffs, long long ld, long long B, int N, double scale_c,
                              double* sigma_out, double* thr_out, hipStream_t st) {
  return run_sigma(coeffs, ld, B, N, scale_c, sigma_out, thr_out, (const double*)nullptr, (double*)nullptr, st);
}

hipError_t launch_median(const double* x, long long ld, long long B, int N, const double* center, double* median_out,
                         hipStream_t st) {
  return run_sigma(x, ld, B, N, 0.0, (double*)nullptr, (double*)nullptr, center, median_out, st);
}

__global__ void __launch_bounds__(256) k_abs_center(const double* __restrict__ x, long long ld, int N,
                                                    const double* __restrict__ center, double* __restrict__ out) {
  const long long b = blockIdx.y;
  const double c = center[b];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x)
    out[b * (long long)N + i] = __builtin_fabs(x[b * ld + i] - c);  // Math.abs(values[i] - median)
}

hipError_t launch_abs_center(const double* x, long long ld, long long B, int N, const double* center, double* out,
                             hipStream_t st) {
  if (B > 65535) return hipErrorInvalidConfiguration;
  const unsigned gx = (unsigned)std::min(std::max((N + 255) / 256, 1), 1024);
  return launch_k<k_abs_center>(dim3(gx, (unsigned)B), dim3(256), 0, st, x, ld, N, center, out);
}

hipError_t launch_seq_std(const double* x, int n, double* out, hipStream_t st) {
  return launch_k<k_seq_std>(dim3(1), dim3(64), 0, st, x, n, out);
}

hipError_t launch_gather_abs(const double* src, const int* idx, int count, double* window, int wsize, int start,
                             hipStream_t st) {
  if (count <= 0) return hipSuccess;
  return launch_k<k_gather_abs>(dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, src, idx, count, window, wsize,
                                start);
}

// WaveletDenoiser thresholds, one per (level, signal): SURE by the sort + exact-tie kernel, the others
// by k_level_threshold.
hipError_t launch_level_threshold(const double* coeffs, long long level_stride, const double* sigma,
                                  const DenoiseConsts& k, long long B, int levels, double* thr, hipStream_t st) {
  if (B <= 0 || levels <= 0) return hipSuccess;
  const dim3 grid((unsigned)B, (unsigned)levels);
  if (k.method == kThrSure) {
    int npow2 = 1;
    while (npow2 < k.n) npow2 <<= 1;
    const int lds = npow2 * (int)sizeof(unsigned long long);
    // (this kernel also has static LDS: raise the limit to what it asks)
    return launch_k<k_sure_threshold, true>(grid, dim3(kSureThreads), lds, st, coeffs, level_stride, sigma, k, B, thr);
  }
  return launch_k<k_level_threshold>(grid, dim3(64), 0, st, coeffs, level_stride, sigma, k, B, thr);
}

template <typename T>
hipError_t launch_threshold(T* c, long long B, long long N, const T* thr, int soft, hipStream_t st) {
  const long long total = B * N;
  const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 65536);
  return launch_k<k_threshold<T>>(dim3(grid), dim3(256), 0, st, c, B, N, thr, soft);
}

template <typename T>
hipError_t launch_fill_uniform(T* x, long long count, unsigned long long seed, long long offset, hipStream_t st) {
  const unsigned grid = (unsigned)std::min<long long>((count + 255) / 256, 65536);
  return launch_k<k_fill_uniform<T>>(dim3(grid), dim3(256), 0, st, x, count, seed, offset);
}

template <typename T>
hipError_t launch_single_haar_batch(const T* x, long long ldx, long long B, int N, T* approx, T* detail,
                                    hipStream_t st) {
  const unsigned gx = (unsigned)std::min(std::max((N + 255) / 256, 1), 1024);
  return launch_k<k_single_haar_batch<T>>(dim3(gx, (unsigned)B), dim3(256), 0, st, x, ldx, N, approx, detail);
}

// AoS <-> SoA layout change (BatchSIMDMODWT.convertToSoA / convertFromSoA, ext/extensions/modwt/
// BatchSIMDMODWT.java:282-308): out[c][r] = in[r][c] for a rows x cols matrix, through 64 x 64 LDS
// tiles (one padding column: conflict-free column reads), coalesced on both sides.  HBM-bound: 2 x
// sizeof(T) bytes per element.
constexpr int kTrTile = 64;
template <typename T>
__global__ void __launch_bounds__(256) k_transpose(const T* __restrict__ in, long long rows, long long cols,
                                                   T* __restrict__ out) {
  __shared__ T tile[kTrTile][kTrTile + 1];
  const long long r0 = (long long)blockIdx.y * kTrTile, c0 = (long long)blockIdx.x * kTrTile;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 64 x 4 threads
#pragma unroll
  for (int k = 0; k < kTrTile; k += 4) {
    const long long r = r0 + ty + k, c = c0 + tx;
    if (r < rows && c < cols) tile[ty + k][tx] = in[r * cols + c];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kTrTile; k += 4) {
    const long long c = c0 + ty + k, r = r0 + tx;  // output row c, column r
    if (r < rows && c < cols) out[c * rows + r] = tile[tx][ty + k];
  }
}

template <typename T>
hipError_t launch_transpose(const T* in, long long rows, long long cols, T* out, hipStream_t st) {
  const dim3 grid((unsigned)((cols + kTrTile - 1) / kTrTile), (unsigned)((rows + kTrTile - 1) / kTrTile));
  if (grid.y > 65535u) return hipErrorInvalidConfiguration;
  return launch_k<k_transpose<T>>(grid, dim3(256), 0, st, in, rows, cols, out);
}

#define VW_INST(T)                                                                                              \
  template hipError_t launch_history_update<T>(const T*, long long, const T*, T*, long long, int, int,         \
                                               hipStream_t);                                                    \
  template hipError_t launch_threshold<T>(T*, long long, long long, const T*, int, hipStream_t);               \
  template hipError_t launch_fill_uniform<T>(T*, long long, unsigned long long, long long, hipStream_t);       \
  template hipError_t launch_single_haar_batch<T>(const T*, long long, long long, int, T*, T*, hipStream_t); \
  template hipError_t launch_transpose<T>(const T*, long long, long long, T*, hipStream_t);
VW_INST(double)
VW_INST(float)
#undef VW_INST

}  // namespace vw
