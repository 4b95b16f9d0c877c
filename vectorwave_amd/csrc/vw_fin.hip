// vw_fin.hip -- com.morphiqlabs.financial on the device: FinancialAnalyzer's four metrics and
// FinancialWaveletAnalyzer's (wavelet) Sharpe ratio, each one launch over a batch of rows.
//
// Every metric is a reduction over the level-1 PERIODIC MODWT of a row (the reference's
// `transform.forward(returns)`), so a workgroup owns one row: the row goes to LDS once, the
// coefficients replace it there (through registers: r and d together do not fit at n = 16384) and
// only the reduced doubles go back to HBM.  The convolution is the EXACT arithmetic of
// vw_modwt1_forward_f64 / vw_modwt1_inverse_f64 (taps * 1/sqrt(2) from the host, separate multiply and
// add, taps ascending; this unit is built with -ffp-contract=off like the others).
//
// Sums: by default one lane walks the coefficients in index order, as the Java loops do
// (bit-identical; the dependent fp64 adds of that walk, not HBM, bound the kernel).  With
// FinArgs::tree every sum is per-thread partials + a wave / workgroup tree (VW_FLAG_TREE_SUMS).
// Maxima and `any` do not depend on the order and are always reduced in parallel.
#include "vw_launch_k.h"

namespace vw {

namespace {

constexpr int kFinWaves = kMaxThreads / 64;
constexpr int kFinRes = 6;                                  // broadcast slots behind the wave partials
// doubles behind the row in LDS: reduction scratch, taps, the waves' edge approximations (k_fin_analyze)
constexpr int kFinScratch = kFinWaves + kFinRes + 2 * kFinMaxTaps + kFinWaves * kFinPerThread;

__device__ __forceinline__ int fin_wrap(int i, int n) {  // ((i % n) + n) % n, i < n
  if (i < 0) {
    i += n;
    if (i < 0) i = ((i % n) + n) % n;
  }
  return i;
}

// Taps from the kernel arguments to LDS (compile-time offsets: a lane-indexed read of a by-value struct would
// copy it to scratch).  The first barrier of the row loop publishes them.
__device__ __forceinline__ void fin_taps_to_lds(const FinArgs& p, double* lo, double* hi) {
#pragma unroll
  for (int l = 0; l < kFinMaxTaps; ++l)
    if ((int)threadIdx.x == l && l < p.L) {
      lo[l] = p.lo[l];
      hi[l] = p.hi[l];
    }
}

// Workgroup sum in a fixed order (lane butterflies, then the waves in order): every thread gets the total.
__device__ __forceinline__ double block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double t = red[0];
  for (int k = 1; k < nw; ++k) t += red[k];
  return t;
}

__device__ __forceinline__ double block_max(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v = __builtin_fmax(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double t = red[0];
  for (int k = 1; k < nw; ++k) t = __builtin_fmax(t, red[k]);
  return t;
}

// Level-1 forward of buf[0..n) at t (ScalarOps.circularConvolveMODWTScalar: sum += signal[(t-l) mod n] * filter[l]).
__device__ __forceinline__ double fin_conv(const double* buf, int n, int t, const double* f, int L) {
  double s = 0.0;
#pragma nounroll
  for (int l = 0; l < L; ++l) s += buf[fin_wrap(t - l, n)] * f[l];
  return s;
}

// FinancialWaveletAnalyzer.calculateSharpeRatio :95-124 from the two sums' results.
__device__ __forceinline__ double fin_sharpe_ratio(double mean, double ssd, int n, double rf) {
  const double sd = __builtin_sqrt(ssd / (n - 1));
  if (sd == 0.0) {
    if (mean == rf) return 0.0;
    return mean > rf ? __builtin_inf() : -__builtin_inf();
  }
  return (mean - rf) / sd;
}

}  // namespace

// FinancialAnalyzer.analyzeCrashAsymmetry / analyzeVolatility / analyzeRegimeTrend / detectAnomalies
// (financial/FinancialAnalyzer.java:52-198) of price row b -> out[0..5)[b].  blockDim.x * kFinPerThread >= n.
__global__ void __launch_bounds__(kMaxThreads) k_fin_analyze(const FinArgs p) {
  extern __shared__ __attribute__((aligned(16))) char fin_smem[];
  const int n = p.N - 1;
  double* buf = reinterpret_cast<double*>(fin_smem);  // [n] returns, then details
  double* red = buf + ((n + 1) & ~1);                 // [kFinWaves + kFinRes]
  double* lo = red + kFinWaves + kFinRes;                   // taps (LDS broadcasts: 60 doubles do not fit the scalar file)
  double* hi = lo + kFinMaxTaps;
  double* edge = hi + kFinMaxTaps;                    // [kFinWaves * kFinPerThread]
  const int tid = threadIdx.x, T = blockDim.x;
  fin_taps_to_lds(p, lo, hi);
  for (long long b = blockIdx.x; b < p.B; b += gridDim.x) {
    const double* row = p.x + b * p.ld;
    // calculateReturns :248-265
    for (int i = tid; i < n; i += T) {
      const double p0 = row[i], p1 = row[i + 1];
      const double r = __builtin_fabs(p0) > 1e-10 ? (p1 - p0) / p0 : 0.0;
      if (p.validate) {
        const unsigned long long flat = (unsigned long long)b * (unsigned long long)p.N + (unsigned long long)i;
        const bool f0 = __builtin_isfinite(p0), f1 = __builtin_isfinite(p1);
        if (!f0) atomicMin(p.bad, flat);
        if (!f1 && i == n - 1) atomicMin(p.bad, flat + 1);
        if (f0 && f1 && !__builtin_isfinite(r)) atomicMin(p.bad, (1ull << 62) | flat);
      }
      buf[i] = r;
    }
    __syncthreads();
    // a[t - 1] for the outputs of lane 0 of every wave; the other lanes take their neighbour's a[t]
    const int nw = T >> 6;
    if (tid < nw * kFinPerThread) {  // edge[k * nw + w]: k = tid / nw, w = tid % nw
      const int t = ((tid % nw) << 6) + (tid / nw) * T;
      if (t >= 1 && t < n) edge[tid] = fin_conv(buf, n, t - 1, lo, p.L);
    }
    __syncthreads();
    // forward: this thread's details stay in registers until every thread has read the returns
    double dreg[kFinPerThread];
    double trend = 0.0;
#pragma unroll
    for (int k = 0; k < kFinPerThread; ++k) {
      const int t = tid + k * T;
      double a1 = 0.0;
      dreg[k] = 0.0;
      if (t < n) {
        dreg[k] = fin_conv(buf, n, t, hi, p.L);
        a1 = fin_conv(buf, n, t, lo, p.L);
      }
      const double up = __shfl_up(a1, 1, 64);
      if (t < n && t >= 1) {  // analyzeRegimeTrend :147-151
        const double a0 = (tid & 63) ? up : edge[k * nw + (tid >> 6)];
        trend = __builtin_fmax(trend, __builtin_fabs(a1 - a0));
      }
    }
    trend = block_max(trend, red);  // (its barriers also end the reads of the returns)
    // counts do not depend on the order: always a tree (exact: small integers)
    double c_pos = 0.0, c_neg = 0.0;
#pragma unroll
    for (int k = 0; k < kFinPerThread; ++k) {  // dreg is 0.0 past the row: counts nothing, adds nothing
      c_pos += dreg[k] > 0 ? 1.0 : 0.0;
      c_neg += dreg[k] < 0 ? 1.0 : 0.0;
    }
    const double npos = block_sum(c_pos, red), nneg = block_sum(c_neg, red);
    double pos, neg, energy, mean, var;
    if (p.tree) {
      double s_pos = 0.0, s_neg = 0.0, s_e = 0.0, s_m = 0.0;
#pragma unroll
      for (int k = 0; k < kFinPerThread; ++k) {
        const double d = dreg[k];
        s_pos += d > 0 ? d : 0.0;
        s_neg += d < 0 ? -d : 0.0;
        s_e += d * d;
        s_m += d;
      }
      pos = block_sum(s_pos, red);
      neg = block_sum(s_neg, red);
      energy = block_sum(s_e, red);
      mean = block_sum(s_m, red) / n;
      double s_v = 0.0;
#pragma unroll
      for (int k = 0; k < kFinPerThread; ++k)
        if (tid + k * T < n) {
          const double diff = dreg[k] - mean;
          s_v += diff * diff;
        }
      var = block_sum(s_v, red);
    } else {
#pragma unroll
      for (int k = 0; k < kFinPerThread; ++k)
        if (tid + k * T < n) buf[tid + k * T] = dreg[k];
      __syncthreads();
      // The reference's loops, in index order.  Its four sums are independent chains: each is walked by
      // lane 0 of another wave (waves of a workgroup sit on different SIMDs; the row rotates the assignment so
      // that the workgroups sharing a compute unit do not all walk on the same SIMD).  pos / neg only ever
      // grow from +0.0, so adding 0.0 for the other sign leaves them bit-identical.
      double* res = red + kFinWaves;  // pos, neg, energy, mean, var
      for (int c = 0; c < 4; ++c) {
        if (tid != (((c + (int)(b & 1023)) % nw) << 6)) continue;
        double acc = 0.0;
        if (c == 0) {
#pragma unroll 8
          for (int i = 0; i < n; ++i) acc += buf[i] > 0 ? buf[i] : 0.0;
        } else if (c == 1) {
#pragma unroll 8
          for (int i = 0; i < n; ++i) acc += buf[i] < 0 ? __builtin_fabs(buf[i]) : 0.0;
        } else if (c == 2) {
#pragma unroll 8
          for (int i = 0; i < n; ++i) acc += buf[i] * buf[i];
        } else {
#pragma unroll 8
          for (int i = 0; i < n; ++i) acc += buf[i];
          const double m = acc / n;
          acc = 0.0;
#pragma unroll 8
          for (int i = 0; i < n; ++i) {
            const double diff = buf[i] - m;
            acc += diff * diff;
          }
          res[3] = m;
          c = 4;  // (acc is the variance sum)
        }
        res[c] = acc;
      }
      __syncthreads();
      pos = res[0];
      neg = res[1];
      energy = res[2];
      mean = res[3];
      var = res[4];
    }
    const double sd = __builtin_sqrt(var / n);
    const double lim = p.k * sd;
    double hit = 0.0;  // (reduced like the maximum: all LDS scratch stays in the dynamic region)
#pragma unroll
    for (int k = 0; k < kFinPerThread; ++k)
      if (tid + k * T < n && __builtin_fabs(dreg[k] - mean) > lim) hit = 1.0;
    hit = block_max(hit, red);
    if (tid == 0) {
      double asym = 0.0;
      if (npos != 0 && nneg != 0) {
        const double pa = pos / npos, na = neg / nneg;
        const double mx = __builtin_fmax(pa, na);
        if (!(mx < 1e-10)) asym = __builtin_fabs(na - pa) / mx;
      }
      p.out[b] = asym;
      p.out[p.B + b] = __builtin_sqrt(energy / n);
      p.out[2 * p.B + b] = n < 2 ? 0.0 : trend;
      p.out[3 * p.B + b] = hit;
      p.out[4 * p.B + b] = sd;
    }
    __syncthreads();  // the next row overwrites buf / red
  }
}

// FinancialWaveletAnalyzer.calculateSharpeRatio (financial/FinancialWaveletAnalyzer.java:95-124, :234-255)
// of returns row b; with p.wavelet, of calculateWaveletSharpeRatio's denoised row (:166-212): level-1
// forward, inverse with an all-zero detail array (MODWTTransform.inverse's `sl[l]*a + sh[l]*0.0` pairs,
// kept as written: they decide signed zeros and turn a non-finite tap product into NaN as the Java does).
__global__ void __launch_bounds__(kMaxThreads) k_fin_sharpe(const FinArgs p) {
  extern __shared__ __attribute__((aligned(16))) char fin_smem[];
  const int n = p.N;
  double* buf = reinterpret_cast<double*>(fin_smem);
  double* red = buf + ((n + 1) & ~1);
  double* lo = red + kFinWaves + kFinRes;
  double* hi = lo + kFinMaxTaps;
  const int tid = threadIdx.x, T = blockDim.x;
  fin_taps_to_lds(p, lo, hi);
  for (long long b = blockIdx.x; b < p.B; b += gridDim.x) {
    const double* row = p.x + b * p.ld;
    double v[kFinPerThread];
#pragma unroll
    for (int k = 0; k < kFinPerThread; ++k) {
      const int t = tid + k * T;
      v[k] = 0.0;
      if (t < n) {
        v[k] = row[t];
        if (p.validate && !__builtin_isfinite(v[k]))
          atomicMin(p.bad, (unsigned long long)b * (unsigned long long)n + (unsigned long long)t);
        buf[t] = v[k];
      }
    }
    __syncthreads();
    if (p.wavelet) {
#pragma unroll
      for (int k = 0; k < kFinPerThread; ++k)
        if (tid + k * T < n) v[k] = fin_conv(buf, n, tid + k * T, lo, p.L);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kFinPerThread; ++k)
        if (tid + k * T < n) buf[tid + k * T] = v[k];
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kFinPerThread; ++k) {
        const int t = tid + k * T;
        if (t < n) {
          double s = 0.0;
#pragma nounroll
          for (int l = 0; l < p.L; ++l) s += lo[l] * buf[(t + l) % n] + hi[l] * 0.0;
          v[k] = s;
        }
      }
      __syncthreads();
      if (!p.tree) {
#pragma unroll
        for (int k = 0; k < kFinPerThread; ++k)
          if (tid + k * T < n) buf[tid + k * T] = v[k];
        __syncthreads();
      }
    }
    if (p.tree) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < kFinPerThread; ++k) s += v[k];  // 0.0 past the row
      const double mean = block_sum(s, red) / n;
      double q = 0.0;
#pragma unroll
      for (int k = 0; k < kFinPerThread; ++k)
        if (tid + k * T < n) {
          const double diff = v[k] - mean;
          q += diff * diff;
        }
      const double ssd = block_sum(q, red);
      if (tid == 0) p.out[b] = fin_sharpe_ratio(mean, ssd, n, p.k);
    } else if (tid == (((int)(b & 1023) % (T >> 6)) << 6)) {  // one lane walks; the row picks its wave (SIMD)
      double s = 0.0;
#pragma unroll 8
      for (int i = 0; i < n; ++i) s += buf[i];
      const double mean = s / n;
      double q = 0.0;
#pragma unroll 8
      for (int i = 0; i < n; ++i) {
        const double diff = buf[i] - mean;
        q += diff * diff;
      }
      p.out[b] = fin_sharpe_ratio(mean, q, n, p.k);
    }
    __syncthreads();
  }
}

static int fin_threads(int n) {
  int t = (n + kFinPerThread - 1) / kFinPerThread;
  t = (t + 63) / 64 * 64;
  return t < 64 ? 64 : t;
}

static int fin_lds(int n) { return (((n + 1) & ~1) + kFinScratch) * (int)sizeof(double); }

hipError_t launch_fin_analyze(const FinArgs& a, hipStream_t st) {
  const int n = a.N - 1, lds = fin_lds(n);
  const unsigned grid = (unsigned)(a.B < (1LL << 20) ? a.B : (1LL << 20));
  return launch_k<k_fin_analyze>(dim3(grid), dim3(fin_threads(n)), lds, st, a);
}

hipError_t launch_fin_sharpe(const FinArgs& a, hipStream_t st) {
  const int lds = fin_lds(a.N);
  const unsigned grid = (unsigned)(a.B < (1LL << 20) ? a.B : (1LL << 20));
  return launch_k<k_fin_sharpe>(dim3(grid), dim3(fin_threads(a.N)), lds, st, a);
}

}  // namespace vw
