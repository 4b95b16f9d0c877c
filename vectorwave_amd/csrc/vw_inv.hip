// vw_inv.hip -- launchers (instantiation unit, once per element type: -DVW_T=double / float) of the fused inverse
// kernels (vw_dev_inv.h) and the register-blocked inverse (vw_blk.h).
#include "vw_launch_k.h"
#include "vw_dev_inv.h"
#include "vw_blk.h"

namespace vw {

// The forms of the fused inverse, in the order the choice tests them.
enum class InvForm { kPair, kTwoBuffer, kBlocked, kPlain6, kPlain8, kFullSlab, kOneBuffer };

template <typename T, int L, int NV>
static InvForm inverse_form(const InvArgs<T>& a) {
  if (a.pair) return InvForm::kPair;     // pairwise sums: k_inverse_fused
  if (a.db) return InvForm::kTwoBuffer;  // sequential sums, two LDS buffers: k_inverse_db
  // register-blocked PERIODIC (host contract; never with NV = 2)
  if (L > 0 && NV != 2 && a.blk) return InvForm::kBlocked;
  // full-slab form of the one-buffer sequential kernel (host: InvArgs::full), short filters at NV = 4 ...
  if (NV == 4 && L > 0 && L <= 8 && a.full) {
    // ... and its PLAIN form (host: InvArgs::plain; the pointers are the executor's), compiled for 6 or 8 waves per SIMD
    if (std::is_same<T, double>::value && a.plain && !a.thr && !a.nf_flag && !a.approx_zero && !a.rev)
      return a.waves == 8 ? InvForm::kPlain8 : InvForm::kPlain6;
    return InvForm::kFullSlab;
  }
  return InvForm::kOneBuffer;  // sequential sums, one LDS buffer: k_inverse_seq
}

template <typename T, int L, bool FMA, int NV>
static hipError_t run_inverse_fused_nv(const InvArgs<T>& a, int threads, int lds, hipStream_t st) {
  const dim3 grid((unsigned)a.B), block(threads);
  // the forms that exist only for some (T, L, NV): inverse_form names them for no other
  constexpr bool kShort = NV == 4 && L > 0 && L <= 8, kF64 = std::is_same<T, double>::value;
  switch (inverse_form<T, L, NV>(a)) {
    case InvForm::kPair: return launch_k<k_inverse_fused<T, L, FMA, NV>>(grid, block, lds, st, a);
    case InvForm::kTwoBuffer: return launch_k<k_inverse_db<T, L, FMA, NV>>(grid, block, lds, st, a);
    case InvForm::kBlocked:
      if constexpr (L > 0 && NV != 2) return launch_k<k_inverse_blk<T, L, FMA, NV>>(grid, block, lds, st, a);
      break;
    case InvForm::kPlain6:
      if constexpr (kShort && kF64) return launch_k<k_inverse_seq<T, L, FMA, NV, true, L, 6, true>>(grid, block, lds, st, a);
      break;
    case InvForm::kPlain8:
      if constexpr (kShort && kF64) return launch_k<k_inverse_seq<T, L, FMA, NV, true, L, 8, true>>(grid, block, lds, st, a);
      break;
    case InvForm::kFullSlab:
      if constexpr (kShort) return launch_k<k_inverse_seq<T, L, FMA, NV, true>>(grid, block, lds, st, a);
      break;
    case InvForm::kOneBuffer: break;
  }
  return launch_k<k_inverse_seq<T, L, FMA, NV>>(grid, block, lds, st, a);
}

template <typename T, int L, bool FMA>
static hipError_t run_inverse_fused(const InvArgs<T>& a, int threads, int lds, int nv, hipStream_t st) {
  if constexpr (L > 0 && L <= 8) {  // NV = 2 (1024 threads): short filters at small batches (host policy)
    if (nv == 2) return run_inverse_fused_nv<T, L, FMA, 2>(a, threads, lds, st);
  }
  return nv <= 4 ? run_inverse_fused_nv<T, L, FMA, 4>(a, threads, lds, st) : run_inverse_fused_nv<T, L, FMA, 8>(a, threads, lds, st);
}

// Two-length banks (InvArgs::taps_hi != taps; the planner's VW_BI route: sequential sums, NV = 4 / 8): each branch
// at its own tap count -- the compile-time pairs of VW_TAP_PAIR_LIST, else the runtime-L kernel with its two counts.
template <typename T, int L, int LH, bool FMA, int NV>
static hipError_t run_inverse_bi_nv(const InvArgs<T>& a, int threads, int lds, hipStream_t st) {
  const dim3 grid((unsigned)a.B), block(threads);
  if (a.db) return launch_k<k_inverse_db<T, L, FMA, NV, LH>>(grid, block, lds, st, a);
  return launch_k<k_inverse_seq<T, L, FMA, NV, false, LH>>(grid, block, lds, st, a);
}

template <typename T>
hipError_t launch_inverse_fused(const InvArgs<T>& a, int threads, int lds, bool fma, int nv, hipStream_t st) {
  if (a.taps_hi != a.taps) {
    if (a.pair || a.blk || nv == 2) return hipErrorInvalidValue;  // not a plan of the two-length route
    return dispatch_tap_pair(a.unrolled, a.taps, a.taps_hi, fma, [&](auto l, auto lh, auto m) {
      return nv <= 4 ? run_inverse_bi_nv<T, l(), lh(), m(), 4>(a, threads, lds, st)
                     : run_inverse_bi_nv<T, l(), lh(), m(), 8>(a, threads, lds, st);
    });
  }
  // unaligned rows / partial slabs: runtime-L kernel
  return dispatch_taps<Unlisted::kRuntimeL>(a.unrolled ? a.taps : 0, fma, [&](auto l, auto m) {
    return run_inverse_fused<T, l(), m()>(a, threads, lds, nv, st);
  });
}
template hipError_t launch_inverse_fused<VW_T>(const InvArgs<VW_T>&, int, int, bool, int, hipStream_t);
}  // namespace vw
