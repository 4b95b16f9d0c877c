// vw_mra.hip -- multiresolution analysis: every additive component of a MODWT in one launch
// (x = S_J + D_1 + ... + D_J; out[0] = S_J, out[c] = D_c), instantiation unit compiled once per element type.
//
// Component c is the masked inverse the engine already has (VectorWaveSwtAdapter.extractLevel,
// core/swt/VectorWaveSwtAdapter.java:576-598: detail_mask = c ? 1 << (c-1) : 0, approx_zero = c != 0).  That inverse
// stages the zeroed planes in LDS and multiplies them tap by tap: 2 J branch passes per component.  Each
// accumulator starts at +0.0 and never becomes -0.0, so a product with a zero input -- +-0 for finite data --
// leaves it as it was, and the pairwise term h*a + g*0 of the ZERO_PADDING sums is the single product.  Hence,
// bit for bit:
//   component 0      = low-pass branch passes at levels J .. 1 on a_J
//   component c > 0  = ONE high-pass branch pass at level c on d_c, then low-pass passes at levels c-1 .. 1
// i.e. J(J+1)/2 + J passes per row instead of 2 J (J+1).  Not for non-finite data (0 * Inf = NaN): the planner
// keeps VW_FLAG_REF_NONFINITE / VW_FLAG_VALIDATE calls on the loop of masked inverses.
//
// Two LDS regions, used ping-pong: a pass reads one region while its sums -- the next level's input, halo
// included -- go to the other, so every pass costs ONE workgroup barrier (k_inverse_db's pattern).  The next
// component's input row is prefetched into registers while the current chain computes.
#include "vw_launch_k.h"
#include "vw_dev_rows.h"

namespace vw {

// Host contract (vw_plan.cpp plan_mra): whole waves; two regions of `region1` elements each holding a row, the
// longest level's halos (both branches' reach) and the left pad; unrolled only for aligned full-slab rows.
template <typename T, int L, bool FMA, int NV>
__global__ void VW_FUSED_BOUNDS(NV, VW_FUSED_W(L, 6)) k_mra(const MraArgs<T> p) {
  constexpr int V = VT<T>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* const R0 = reinterpret_cast<T*>(smem) + p.hlpad;
  T* const R1 = R0 + p.region1;
  const int N = p.N;
  const int nvec = (N + V - 1) / V;
  const bool vec_ok = (L > 0) || p.vec_io != 0;
  const size_t plane = (size_t)p.B * (size_t)N;

  // W: the region the next writer fills.  Invariant: every pass is preceded by a barrier, reads the region
  // written last and leaves W at the other one -- whose last reads lie before that barrier.
  T* W = R0;
  T* O = R1;
  for (long long b = blockIdx.x; b < p.B; b += gridDim.x) {
    T acc[NV][V];
    T nxt[NV][V];
    load_row_regs<T, NV>(nxt, p.approx + (size_t)b * (size_t)N, N, nvec, vec_ok, false);
    for (int c = 0; c <= p.J; ++c) {
      const int jtop = c == 0 ? p.J : c;
      wait_vmem();  // this component's input row (and the previous component's stores)
      regs_to_level<T, L, NV>(W, nxt, nvec, N, p.lv[jtop - 1], 0, (const T*)nullptr);
      if (c < p.J)  // d_{c+1}, for the next component, while this chain computes
        load_row_regs<T, NV>(nxt, p.details + (size_t)c * plane + (size_t)b * (size_t)N, N, nvec, vec_ok, false);
      for (int j = jtop; j >= 1; --j) {
        const LevelDesc lv = p.lv[j - 1];
        const bool high = c > 0 && j == jtop;
        lds_barrier();  // W = the level-j input + halo; every read of O done
        { T* t = W; W = O; O = t; }
        zero_regs<T, NV>(acc);
        if (high) inv_row<T, L, FMA, NV>(O, nvec, lv.s, lv.dir_d, lv.off_d, p.hi, p.taps, p.level_ct, acc);
        else inv_row<T, L, FMA, NV>(O, nvec, lv.s, lv.dir_a, lv.off_a, p.lo, p.taps, p.level_ct, acc);
        if (j > 1) regs_to_level<T, L, NV>(W, acc, nvec, N, p.lv[j - 2], 0, (const T*)nullptr);
      }
      T* const dst = p.out + (size_t)c * plane + (size_t)b * (size_t)N;
      for_vecs<L, NV>(nvec, [&](int k, int w) { store_vec<VW_INV_STORE_AUX>(dst, w * V, N, vec_ok, acc[k]); });
    }
  }
}

template <typename T>
hipError_t launch_mra(const MraArgs<T>& a, int threads, int lds, bool fma, int nv, int grid, hipStream_t st) {
  if (threads <= 0 || threads % 64 != 0 || grid <= 0 || (nv != 4 && nv != 8)) return hipErrorInvalidConfiguration;
  auto run = [&](auto l, auto m) {
    if (nv <= 4) return launch_k<k_mra<T, l(), m(), 4>>(dim3((unsigned)grid), dim3(threads), lds, st, a);
    return launch_k<k_mra<T, l(), m(), 8>>(dim3((unsigned)grid), dim3(threads), lds, st, a);
  };
  // Tap-unrolled bodies up to kMraUnrollMax (the energy unit's precedent; plan_mra names no kernel this unit lacks);
  // unaligned rows and partial slabs take the runtime-L body.
  if (a.unrolled) return dispatch_taps<Unlisted::kInvalidConfiguration, kMraUnrollMax>(a.taps, fma, run);
  return with_fma(fma, [&](auto m) { return run(std::integral_constant<int, 0>{}, m); });
}
template hipError_t launch_mra<VW_T>(const MraArgs<VW_T>&, int, int, bool, int, int, hipStream_t);

}  // namespace vw
