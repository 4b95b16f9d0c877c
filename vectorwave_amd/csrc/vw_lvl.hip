// vw_lvl.hip -- launchers (instantiation unit, once per element type: -DVW_T=double / float) of the per-level
// path's kernels (vw_dev_lvl.h): tiled levels, column sweeps, and (vw_multi.inc) the multi-level tiles.
#include "vw_launch_k.h"
#include "vw_dev_lvl.h"

namespace vw {

template <typename T, bool INV>
static hipError_t dispatch_level(const LevelArgs<T>& a, int lds, bool fma, hipStream_t st) {
  const dim3 grid((unsigned)((a.N + a.tile - 1) / a.tile), (unsigned)a.B), block(256);
  return dispatch_taps<Unlisted::kRuntimeL>(a.taps, fma, [&](auto l, auto m) {
    if constexpr (INV) return launch_k<k_inverse_level<T, l(), m()>>(grid, block, lds, st, a);
    else return launch_k<k_forward_level<T, l(), m()>>(grid, block, lds, st, a);
  });
}

// Column sweeps (k_forward_sweep / k_inverse_sweep): one thread per (signal, column, q-chunk).
template <typename T>
static unsigned sweep_blocks(const LevelArgs<T>& a) {
  const long long s = a.lv.s, qn = (a.N + s - 1) / s, chunks = (qn + a.tile - 1) / a.tile;
  return (unsigned)((a.B * s * chunks + 255) / 256);
}

template <typename T>
hipError_t launch_forward_sweep(const LevelArgs<T>& a, bool fma, hipStream_t st) {
  // runtime-L filters use the tiled kernel
  return dispatch_taps<Unlisted::kInvalidValue>(a.taps, fma, [&](auto l, auto m) {
    return launch_k<k_forward_sweep<T, l(), m()>>(dim3(sweep_blocks(a)), dim3(256), 0, st, a);
  });
}
template <typename T>
hipError_t launch_inverse_sweep(const LevelArgs<T>& a, bool fma, hipStream_t st) {
  return dispatch_taps<Unlisted::kInvalidValue>(a.taps, fma, [&](auto l, auto m) {
    const dim3 g(sweep_blocks(a)), blk(256);
    const bool da = a.lv.dir_a > 0, dd = a.lv.dir_d > 0;
    if (da && dd) return launch_k<k_inverse_sweep<T, l(), m(), 1, 1>>(g, blk, 0, st, a);
    if (da) return launch_k<k_inverse_sweep<T, l(), m(), 1, -1>>(g, blk, 0, st, a);
    if (dd) return launch_k<k_inverse_sweep<T, l(), m(), -1, 1>>(g, blk, 0, st, a);
    return launch_k<k_inverse_sweep<T, l(), m(), -1, -1>>(g, blk, 0, st, a);
  });
}
template hipError_t launch_forward_sweep<VW_T>(const LevelArgs<VW_T>&, bool, hipStream_t);
template hipError_t launch_inverse_sweep<VW_T>(const LevelArgs<VW_T>&, bool, hipStream_t);

// Two / three inverse levels per launch (k_inverse_sweep2 / k_inverse_sweep3): one workgroup per (signal,
// R-residue block, u-chunk) of 4R / 12R threads.  KA = 8 or 16 outputs per thread and step; a block
// (G*KA positions) must cover the reach of the levels below the top, and the rings must fit LDS
// (the host applies the same rule: vw_plan.cpp sweepg_plan).
template <typename T, int L, bool FMA, int KA, int R, int G>
static hipError_t run_inverse_sweepg(const LevelArgs<T>& a, hipStream_t st) {
  constexpr int KMIN = (G == 2 ? 1 : 2) * (L - 1);
  constexpr bool fits = (G == 2 ? 1 : 2) * 3 * G * KA * R * (int)sizeof(T) <= kLdsBytes;
  if constexpr (G * KA >= KMIN && fits) {
    const long long h = a.lv.s / G, nu = a.N / h, nch = (nu + a.tile - 1) / a.tile;
    const long long groups = a.B * (h / R) * nch;
    if constexpr (G == 2) return launch_k<k_inverse_sweep2<T, L, FMA, KA, R>>(dim3((unsigned)groups), dim3(4 * R), 0, st, a);
    else return launch_k<k_inverse_sweep3<T, L, FMA, KA, R>>(dim3((unsigned)groups), dim3(12 * R), 0, st, a);
  } else {
    return hipErrorInvalidValue;
  }
}

template <typename T, int L, bool FMA, int G>
static hipError_t run_inverse_sweepg_k(const LevelArgs<T>& a, int ka, int R, hipStream_t st) {
  if (ka == 8) return R == 64 ? run_inverse_sweepg<T, L, FMA, 8, 64, G>(a, st) : run_inverse_sweepg<T, L, FMA, 8, 32, G>(a, st);
  return R == 64 ? run_inverse_sweepg<T, L, FMA, 16, 64, G>(a, st) : run_inverse_sweepg<T, L, FMA, 16, 32, G>(a, st);
}

template <typename T>
hipError_t launch_inverse_sweepg(const LevelArgs<T>& a, int levels, int ka, int R, bool fma, hipStream_t st) {
  if (R != 64 && R != 32) return hipErrorInvalidValue;
  return dispatch_taps<Unlisted::kInvalidValue>(a.taps, fma, [&](auto l, auto m) {
    return levels == 2 ? run_inverse_sweepg_k<T, l(), m(), 2>(a, ka, R, st) : run_inverse_sweepg_k<T, l(), m(), 4>(a, ka, R, st);
  });
}
template hipError_t launch_inverse_sweepg<VW_T>(const LevelArgs<VW_T>&, int, int, int, bool, hipStream_t);

template <typename T>
hipError_t launch_forward_level(const LevelArgs<T>& a, int lds, bool fma, hipStream_t st) {
  return dispatch_level<T, false>(a, lds, fma, st);
}
template <typename T>
hipError_t launch_inverse_level(const LevelArgs<T>& a, int lds, bool fma, hipStream_t st) {
  return dispatch_level<T, true>(a, lds, fma, st);
}
template hipError_t launch_forward_level<VW_T>(const LevelArgs<VW_T>&, int, bool, hipStream_t);
template hipError_t launch_inverse_level<VW_T>(const LevelArgs<VW_T>&, int, bool, hipStream_t);
}  // namespace vw

#include "vw_multi.inc"
