// vw_icwt.hip -- batched inverse continuous wavelet transform (InverseCWT.reconstruct, cwt/InverseCWT.java),
// instantiation unit compiled once per element type.
//
//   SUM     out[b][tau] = ( sum_j weight_j * ( sum_{k=0}^{K_j-1} w_j[k] * z_{b,plane_j}[(tau + o_j + k) mod wrap] ) ) / divisor
//
// with z zero on [N, wrap), k ascending into one accumulator per descriptor that starts at +0.0, j ascending into
// one outer accumulator that starts at +0.0: the weighted sum of circular convolutions that
// reconstructInternalRealFFT (:225-270) evaluates by FFT (o_j = -d_max, w_j[k] = g_j(d_max - k), weight_j =
// weights[j] / a_j, wrap = nextPowerOfTwo(N), divisor = C_psi).
//
// k_icwt: one workgroup per (row, time tile), looping over the call's descriptors.  For each it stages the plane's
// tile plus the K_j - 1 overhang into LDS in k_cwt's layout (cwt_slot, cwt_chunks), the wrap and the zero region
// resolved there, slides k_cwt's two-chunk register window over it into acc[NV], and folds acc into total[NV].  The
// S planes are read once, one row is written.  The taps are wave-uniform and read through scalar loads.
//
//   DIRECT  reconstructInternalRealDirect (:283-311) literally: per output t one accumulator over the descriptors
//           and b ascending, sum += ((c * w_j[t - b + N - 1]) * weight_j) / scale_j, terms with |c| < 1e-10 skipped
//           (a NaN is not), then / divisor.
//
// k_icwt_direct: one thread per output, coefficients and table straight from memory (rows under 128 samples).
#include "vw_cwt_dev.h"

#ifndef VW_T
#error "compile with -DVW_T=double or -DVW_T=float"
#endif

namespace vw {

template <typename T, bool FMA>
__global__ void __launch_bounds__(kCwtThreads)
    k_icwt(const IcwtArgs<T> p, const IcwtScaleDev<T>* __restrict__ sc, const T* __restrict__ taps) {
  // (the table as a restrict argument of its own, as k_cwt: the wave-uniform taps stay scalar loads)
  constexpr int NV = kCwtChunkBytes / (int)sizeof(T);
  constexpr int V = NV / 2;
  struct alignas(16) Vec { T v[V]; };
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* const lds = reinterpret_cast<T*>(smem);
  const int tid = threadIdx.x, threads = blockDim.x;
  const int tile = threads * NV;
  const long long items = p.B * (long long)p.ntiles;

  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const long long b = w / p.ntiles;
    const long long tau0 = (w % p.ntiles) * (long long)tile;
    const T* __restrict__ planes = p.coef + (size_t)b * (size_t)p.S * (size_t)p.ldc;

    T total[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) total[v] = T(0);

    for (int j = 0; j < p.nsc; ++j) {
      const IcwtScaleDev<T> d = sc[j];
      const int K = d.taps;
      const int chunks = cwt_chunks(threads, K, NV);
      const T* __restrict__ z = planes + (size_t)d.plane * (size_t)p.ldc;

      // staged element e is z[(tau0 + o_j + e) mod wrap], zero on [N, wrap) (cwt_ext's kCwtWrapZero read): one
      // modulo per thread, then steps of `threads`
      long long m = (tau0 + d.window + tid) % p.wrap;
      if (m < 0) m += p.wrap;
      for (int e = tid; e < chunks * NV; e += threads) {
        lds[cwt_slot<NV>(e, chunks)] = m < p.N ? z[m] : T(0);
        m += threads;
        while (m >= p.wrap) m -= p.wrap;
      }
      __syncthreads();

      const Vec* const plane0 = reinterpret_cast<const Vec*>(lds);
      const Vec* const plane1 = plane0 + chunks;
      const T* __restrict__ wj = taps + d.tap_begin;

      T win[2 * NV];
      T acc[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[v] = T(0);
      auto load_chunk = [&](int q, T* dst) {
        const Vec a = plane0[q], c = plane1[q];
#pragma unroll
        for (int i = 0; i < V; ++i) { dst[i] = a.v[i]; dst[V + i] = c.v[i]; }
      };
      auto tap = [&](int k, int kk) {  // tap k = k0 + kk on window elements kk .. kk + NV - 1
        const T cw = wj[k];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = FMA ? fma(win[kk + v], cw, acc[v]) : acc[v] + win[kk + v] * cw;
      };

      load_chunk(tid, win);
      int k0 = 0;
      for (; k0 + NV <= K; k0 += NV) {
        load_chunk(tid + k0 / NV + 1, win + NV);
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) tap(k0 + kk, kk);
#pragma unroll
        for (int v = 0; v < NV; ++v) win[v] = win[NV + v];
      }
      if (k0 < K) {  // the last K % NV taps (wave-uniform bounds): a tap past K would multiply a staged value
        load_chunk(tid + k0 / NV + 1, win + NV);
#pragma unroll
        for (int kk = 0; kk < NV - 1; ++kk)
          if (k0 + kk < K) tap(k0 + kk, kk);
      }

      const T wt = d.weight;
#pragma unroll
      for (int v = 0; v < NV; ++v) total[v] = FMA ? fma(acc[v], wt, total[v]) : total[v] + acc[v] * wt;
      __syncthreads();  // the next descriptor restages the tile
    }

    const long long tau = tau0 + (long long)tid * NV;
    T* const orow = p.out + (size_t)b * (size_t)p.ldo;
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (tau + v < p.N) orow[tau + v] = total[v] / p.divisor;
  }
}

template <typename T>
__global__ void __launch_bounds__(kIcwtDirectThreads)
    k_icwt_direct(const IcwtArgs<T> p, const IcwtScaleDev<T>* __restrict__ sc, const T* __restrict__ taps) {
  const long long outputs = p.B * (long long)p.N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < outputs; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / p.N;
    const int t = (int)(i % p.N);
    const T* __restrict__ planes = p.coef + (size_t)b * (size_t)p.S * (size_t)p.ldc;
    T sum = T(0);
    for (int j = 0; j < p.nsc; ++j) {
      const IcwtScaleDev<T> d = sc[j];
      const T* __restrict__ z = planes + (size_t)d.plane * (size_t)p.ldc;
      const T* __restrict__ wt = taps + d.tap_begin + (p.N - 1) + t;  // w_j[t - bb + N - 1] = wt[-bb]
      for (int bb = 0; bb < p.N; ++bb) {
        const T c = z[bb];
        if (fabs(c) < T(1e-10)) continue;
        sum = sum + ((c * wt[-bb]) * d.weight) / d.scale;
      }
    }
    p.out[(size_t)b * (size_t)p.ldo + t] = sum / p.divisor;
  }
}

template <typename T>
hipError_t launch_icwt(const IcwtArgs<T>& a, int threads, int lds, bool fma, int grid, hipStream_t st) {
  if (threads < 64 || threads > kCwtThreads || threads % 64 != 0 || grid <= 0 || grid > kCwtMaxGrid || lds <= 0 ||
      lds > kLdsBytes || a.nsc <= 0 || a.ntiles <= 0 || a.wrap < a.N)
    return hipErrorInvalidConfiguration;
  return with_fma(fma, [&](auto m) {
    return launch_k<k_icwt<T, decltype(m)::value>>(dim3((unsigned)grid), dim3(threads), lds, st, a, a.sc, a.taps);
  });
}
template hipError_t launch_icwt<VW_T>(const IcwtArgs<VW_T>&, int, int, bool, int, hipStream_t);

template <typename T>
hipError_t launch_icwt_direct(const IcwtArgs<T>& a, hipStream_t st) {
  if (a.nsc <= 0 || a.N <= 0 || a.B <= 0) return hipErrorInvalidConfiguration;
  const long long blocks = (a.B * (long long)a.N + kIcwtDirectThreads - 1) / kIcwtDirectThreads;
  const unsigned grid = (unsigned)(blocks < kCwtMaxGrid ? blocks : kCwtMaxGrid);
  return launch_k<k_icwt_direct<T>>(dim3(grid), dim3(kIcwtDirectThreads), 0, st, a, a.sc, a.taps);
}
template hipError_t launch_icwt_direct<VW_T>(const IcwtArgs<VW_T>&, hipStream_t);

}  // namespace vw
