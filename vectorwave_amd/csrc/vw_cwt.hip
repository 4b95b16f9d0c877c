// vw_cwt.hip -- batched continuous wavelet transform as fixed-order correlations of a row with one table per scale,
// instantiation unit compiled once per element type.
//
//   out[b][s][tau] = ( sum_{k=0}^{K_s-1} w_s[k] * ext(x_b, tau + o_s + k) ) / q_s
//
// with k ascending and one accumulator that starts at +0.0: CWTTransform.analyzeDirect / analyzeDirectComplex
// (cwt/CWTTransform.java:120-218, t = k - H ascending, w_s[k] = psi(-(k-H)/s)/sqrt(s), o_s = -H, q_s = 1) and, with
// ext = kCwtWrapZero, o_s = +H and q_s = sqrt(s), what analyzeFFT (:223-318) computes by FFT.  The real and the
// imaginary table feed independent sums of the same window.
//
// One workgroup per (row, time tile, scale), the scales heaviest first.  The workgroup stages the extended tile
// ext(x, tau0 + o_s + e), e in [0, chunks * NV), into LDS once -- the extension is resolved there, the tap loop has
// no index logic.  A thread owns NV adjacent outputs (one 32-byte chunk) and slides a window of two chunks over
// the staged tile: one chunk read (two 16-byte LDS reads) per NV taps feeds NV * NV multiplies, 2 NV * NV with a
// complex table.  The taps are wave-uniform and read through scalar loads.  Each output keeps its own k order,
// so without FMA the sums are the reference's bit for bit.
#include "vw_cwt_dev.h"

#ifndef VW_T
#error "compile with -DVW_T=double or -DVW_T=float"
#endif

namespace vw {

template <typename T, bool CPLX, bool FMA>
__global__ void __launch_bounds__(kCwtThreads)
    k_cwt(const CwtArgs<T> p, const CwtScaleDev<T>* __restrict__ sc, const T* __restrict__ taps_re,
          const T* __restrict__ taps_im) {
  // (the tables as restrict arguments of their own: the compiler then knows the output stores leave them alone
  // and reads the wave-uniform taps through scalar loads)
  constexpr int NV = kCwtChunkBytes / (int)sizeof(T);
  constexpr int V = NV / 2;
  struct alignas(16) Vec { T v[V]; };
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* const lds = reinterpret_cast<T*>(smem);
  const int tid = threadIdx.x, threads = blockDim.x;
  const int tile = threads * NV;
  const long long items = (long long)p.nsc * p.ntiles;
  const long long total = items * p.B;

  // work item w: all rows of the heaviest scale's first tile, then its next tile, ..., then the next scale
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const long long item = w / p.B, b = w % p.B;
    const CwtScaleDev<T> d = sc[item / p.ntiles];
    const int K = d.taps;
    const long long tau0 = (item % p.ntiles) * (long long)tile;
    const int chunks = cwt_chunks(threads, K, NV);
    const T* __restrict__ xrow = p.x + (size_t)b * (size_t)p.ldx;

    const long long g0 = tau0 + d.window;
    for (int e = tid; e < chunks * NV; e += threads) lds[cwt_slot<NV>(e, chunks)] = cwt_ext(xrow, g0 + e, p.N, p.ext, p.wrap);
    __syncthreads();

    const Vec* const plane0 = reinterpret_cast<const Vec*>(lds);
    const Vec* const plane1 = plane0 + chunks;
    const T* __restrict__ wre = taps_re + d.tap_begin;
    const T* __restrict__ wim = CPLX ? taps_im + d.tap_begin : nullptr;

    T win[2 * NV];
    T re[NV], im[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) re[v] = im[v] = T(0);
    auto load_chunk = [&](int q, T* dst) {
      const Vec a = plane0[q], c = plane1[q];
#pragma unroll
      for (int i = 0; i < V; ++i) { dst[i] = a.v[i]; dst[V + i] = c.v[i]; }
    };
    auto tap = [&](int k, int kk) {  // tap k = k0 + kk on window elements kk .. kk + NV - 1
      const T cr = wre[k];
#pragma unroll
      for (int v = 0; v < NV; ++v) re[v] = FMA ? fma(win[kk + v], cr, re[v]) : re[v] + win[kk + v] * cr;
      if constexpr (CPLX) {
        const T ci = wim[k];
#pragma unroll
        for (int v = 0; v < NV; ++v) im[v] = FMA ? fma(win[kk + v], ci, im[v]) : im[v] + win[kk + v] * ci;
      }
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

    const long long tau = tau0 + (long long)tid * NV;
    const size_t row = ((size_t)b * (size_t)p.S + (size_t)d.scale) * (size_t)p.N;
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (tau + v < p.N) {
        p.out_re[row + tau + v] = re[v] / d.divisor;
        if constexpr (CPLX) p.out_im[row + tau + v] = im[v] / d.divisor;
      }
    __syncthreads();  // the next item restages the tile
  }
}

template <typename T, bool CPLX, bool FMA>
static hipError_t run_cwt(const CwtArgs<T>& a, int threads, int lds, int grid, hipStream_t st) {
  return launch_k<k_cwt<T, CPLX, FMA>>(dim3((unsigned)grid), dim3(threads), lds, st, a, a.sc, a.taps_re, a.taps_im);
}

template <typename T>
hipError_t launch_cwt(const CwtArgs<T>& a, int threads, int lds, bool cplx, bool fma, int grid, hipStream_t st) {
  if (threads < 64 || threads > kCwtThreads || threads % 64 != 0 || grid <= 0 || grid > kCwtMaxGrid || lds <= 0 ||
      lds > kLdsBytes || a.nsc <= 0 || a.ntiles <= 0)
    return hipErrorInvalidConfiguration;
  if (cplx) return fma ? run_cwt<T, true, true>(a, threads, lds, grid, st) : run_cwt<T, true, false>(a, threads, lds, grid, st);
  return fma ? run_cwt<T, false, true>(a, threads, lds, grid, st) : run_cwt<T, false, false>(a, threads, lds, grid, st);
}
template hipError_t launch_cwt<VW_T>(const CwtArgs<VW_T>&, int, int, bool, bool, int, hipStream_t);

}  // namespace vw
