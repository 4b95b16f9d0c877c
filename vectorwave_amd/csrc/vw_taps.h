// vw_taps.h -- which kernel instantiations exist, as plain host code: read by the launcher units (their
// dispatch switches) and by the planner (vw_plan.cpp), so neither can name a kernel the other lacks.
#pragma once

namespace vw {

// Unrolled tap counts; other L use the runtime-L kernels.  Dev builds may restrict the list:
// make DEV_TAPS='X(8)' (the runtime-L kernel still covers every other L).
#ifdef VW_DEV_TAPS
#define VW_TAP_LIST(X) VW_DEV_TAPS(X)
#else
#define VW_TAP_LIST(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(18) X(20) X(24) X(30)
#endif

// Which compile-time tap counts have unrolled kernels; others use the runtime-L kernel.
inline bool has_unrolled_taps(int L) {
  switch (L) {
#define VW_CASE(n) case n: return true;
    VW_TAP_LIST(VW_CASE)
#undef VW_CASE
    default: return false;
  }
}

// Banks with two filter lengths (biorthogonal): (low-pass, high-pass) tap counts with compile-time instantiations
// of the two-length fused forward (vw_fwd.hip launch_forward_fused) and sequential inverses (vw_inv.hip
// launch_inverse_fused) -- bior4.4 / rbio4.4 and bior2.2 / rbio2.2, analysis and synthesis pairs alike; read by
// both launchers and by the planner (has_unrolled_pair).  Every other pair runs the runtime-L bodies with its two
// counts (VW_BI bit 2), or the padded route.
#define VW_TAP_PAIR_LIST(X) X(7, 9) X(9, 7) X(3, 5) X(5, 3)
inline bool has_unrolled_pair(int Llo, int Lhi) {
#define VW_CASE(a, b) if (Llo == a && Lhi == b) return true;
  VW_TAP_PAIR_LIST(VW_CASE)
#undef VW_CASE
  return false;
}

// Matrix-core fp32 kernels (vw_mfma.hip): which (L, N) are instantiated, the halo a level set needs, and
// the LDS floats of the kernels' padded level region for elements [0, n) (the tap table follows it).
#ifndef VW_MFMA_PAD_SHIFT
#define VW_MFMA_PAD_SHIFT 3
#endif
inline bool mfma_supported(int L, long long N) {
  return (L == 30 || L == 16) && (N == 2048 || N == 4096 || N == 8192);
}
inline int mfma_halo(int L, int J) { return (4 * ((L + 15 + 3) / 4) - 16) << (J - 1); }
inline int mfma_region(int n) { return n == 0 ? 0 : (n - 1) + ((n - 1) >> VW_MFMA_PAD_SHIFT) + 1; }

}  // namespace vw
