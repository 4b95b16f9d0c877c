// vw_fwd.hip -- launchers (instantiation unit, once per element type: -DVW_T=double / float) of the fused forward
// kernels (vw_dev_fwd.h) and the register-blocked forward (vw_blk.h).
#include "vw_launch_k.h"
#include "vw_dev_fwd.h"
#include "vw_blk.h"
#include <algorithm>

namespace vw {

template <typename T, int L, bool FMA, int NV>
static hipError_t run_forward_fused_nv(const FwdArgs<T>& a, int threads, int lds, hipStream_t st) {
  const dim3 grid((unsigned)a.B), block(threads);
  if (a.hist[0] != nullptr) return launch_k<k_forward_fused<T, L, FMA, NV, true>>(grid, block, lds, st, a);
  return launch_k<k_forward_fused<T, L, FMA, NV, false>>(grid, block, lds, st, a);
}

template <typename T, int L, bool FMA>
static hipError_t run_forward_fused(const FwdArgs<T>& a, int threads, int lds, int nv, hipStream_t st) {
  if constexpr (L > 0 && L <= 8) {  // NV = 2 (1024 threads): short filters at small batches (host policy)
    if (nv == 2) return run_forward_fused_nv<T, L, FMA, 2>(a, threads, lds, st);
  }
  return nv <= 4 ? run_forward_fused_nv<T, L, FMA, 4>(a, threads, lds, st) : run_forward_fused_nv<T, L, FMA, 8>(a, threads, lds, st);
}

template <typename T>
hipError_t launch_forward_fused(const FwdArgs<T>& a, int threads, int lds, bool fma, int nv, hipStream_t st) {
  // Two-length banks (FwdArgs::taps_hi != taps; the planner's VW_BI route: no history, NV = 4 / 8): the compile-time
  // pairs of VW_TAP_PAIR_LIST, else the runtime-L kernel with its two counts.
  if (a.taps_hi != a.taps) {
    if (a.hist[0] != nullptr || nv == 2) return hipErrorInvalidValue;  // not a plan of the two-length route
    return dispatch_tap_pair(a.unrolled, a.taps, a.taps_hi, fma, [&](auto l, auto lh, auto m) {
      const dim3 grid((unsigned)a.B), block(threads);
      if (nv <= 4) return launch_k<k_forward_fused<T, l(), m(), 4, false, lh()>>(grid, block, lds, st, a);
      return launch_k<k_forward_fused<T, l(), m(), 8, false, lh()>>(grid, block, lds, st, a);
    });
  }
  // unaligned rows / partial slabs: runtime-L kernel
  return dispatch_taps<Unlisted::kRuntimeL>(a.unrolled ? a.taps : 0, fma, [&](auto l, auto m) {
    return run_forward_fused<T, l(), m()>(a, threads, lds, nv, st);
  });
}
template hipError_t launch_forward_fused<VW_T>(const FwdArgs<VW_T>&, int, int, bool, int, hipStream_t);

// Register-blocked PERIODIC forward (k_forward_blk), unrolled tap counts only.
template <typename T>
hipError_t launch_forward_blk(const FwdArgs<T>& a, int threads, int lds, bool fma, int nv, hipStream_t st) {
  return dispatch_taps<Unlisted::kNotSupported>(a.taps, fma, [&](auto l, auto m) {
    const dim3 grid((unsigned)a.B), block(threads);
    if (nv <= 4) return launch_k<k_forward_blk<T, l(), m(), 4>>(grid, block, lds, st, a);
    return launch_k<k_forward_blk<T, l(), m(), 8>>(grid, block, lds, st, a);
  });
}
template hipError_t launch_forward_blk<VW_T>(const FwdArgs<VW_T>&, int, int, bool, int, hipStream_t);

// Persistent forward (k_forward_persist): as many workgroups as are resident at once, each walking
// signals blockIdx.x + k*gridDim.x.  The resident count comes from the occupancy API (LDS-bound).
template <typename T, int L, bool FMA, int NV, bool FULL>
static hipError_t run_forward_persist(const FwdArgs<T>& a, int threads, int lds, hipStream_t st) {
  constexpr auto k = k_forward_persist<T, L, FMA, NV, FULL>;
  hipError_t e;
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
  }
  // resident workgroups per CU: one occupancy query per (threads, LDS) shape, not one per launch
  static int q_threads = -1, q_lds = -1, q_per_cu = 0;
  if (threads != q_threads || lds != q_lds) {
    int per_cu = 0;
    if ((e = lds_limit_k<k>(lds)) != hipSuccess) return e;  // the query counts against the raised limit
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, threads, lds)) != hipSuccess) return e;
    q_threads = threads; q_lds = lds; q_per_cu = per_cu;
  }
  const int per_cu = q_per_cu;
  if (per_cu < 1) return hipErrorInvalidConfiguration;
  const long long grid = std::min<long long>(a.B, (long long)per_cu * cus);
  return launch_k<k>(dim3((unsigned)grid), dim3(threads), lds, st, a);
}

template <typename T>
hipError_t launch_forward_persist(const FwdArgs<T>& a, int threads, int lds, bool fma, int nv, hipStream_t st) {
  (void)nv;  // NV = 4 only (host contract)
  return dispatch_taps<Unlisted::kNotSupported>(a.taps, fma, [&](auto l, auto m) {
    // the contract makes every slab full: the full-slab form unless VW_LEVEL_CT=0 asks for the checked one
    return a.level_ct ? run_forward_persist<T, l(), m(), 4, true>(a, threads, lds, st)
                      : run_forward_persist<T, l(), m(), 4, false>(a, threads, lds, st);
  });
}
template hipError_t launch_forward_persist<VW_T>(const FwdArgs<VW_T>&, int, int, bool, int, hipStream_t);
}  // namespace vw
