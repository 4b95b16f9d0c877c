#pragma once
// vw_blk.h -- the register-blocked PERIODIC kernels for long filters (k_forward_blk / k_inverse_blk) and
// their shared pieces, on vw_dev_core.h's helpers (VT, vmadd, static_for, lds_base, the row transfers) and, for the
// levels with s < V, vw_dev_rows.h's row bodies.  Included by the units that launch the two kernels and by
// vw_dev_lvl.h, whose k_inverse_multi borrows BlkC.
//
// Three things are stated once here:
//   * the padded layout rule is blk_pad (vw_internal.h, shared with the planner); BlkC is its
//     compile-time form;
//   * the tap loops are blk_inv_taps / blk_fwd_taps; the ways of reading LDS (per lane, compile-time
//     offsets, wave-uniform offsets, immediates off a laundered base) are readers passed to them;
//   * the dispatch on a compile-time vector stride is blk_stride.
#include "vw_dev_rows.h"

#pragma clang fp contract(off)

namespace vw {

// ---------------------------------------------------------------------------------------------
// Register-blocked PERIODIC kernels for long filters (L > 8: sym8, coif5, ...).  At a level with
// spacing s >= V (vector stride m = s/V) a thread owns the NV output vectors vb, vb+m, .., vb+(NV-1)m
// of a block of m columns; they read the same input vectors shifted by one tap, so a branch costs
// NV+L-1 LDS reads instead of NV*L (33 vs 120 at L = 30): the per-level LDS read traffic, which bounds
// the one-vector-per-tap kernels for long filters, drops ~3.6x.  The block mapping alone would put
// 4..16 lanes of one ds_read_b128 lane group on the same banks, so every level input is written into
// LDS in a padded layout chosen for that level (blk_pad, vw_internal.h), under which the reads are
// conflict-free (modelled with the gfx950 lane groups of the microarchitecture guide's LDS table).
// Levels with s < V run the register-window code in the standard mapping.  Per output the taps run
// i ascending (forward: ScalarOps.java:707-719; inverse: approximation branch then detail branch,
// MultiLevelMODWTTransform.java:576-589): the reference's sums bit for bit in EXACT mode.
__device__ __forceinline__ int blk_phys(const BlkLayout& lo, int u) { return u + (u >> lo.sh) * lo.pad; }

template <typename T>
__device__ __forceinline__ void blk_store(T* R, const BlkLayout& lo, int u, const typename VT<T>::v& o) {
  *reinterpret_cast<typename VT<T>::v*>(R + blk_phys(lo, u) * VT<T>::V) = o;
}

// the 16-byte vector at p
template <typename T>
__device__ __forceinline__ typename VT<T>::v blk_load(const T* p) {
  return *reinterpret_cast<const typename VT<T>::v*>(p);
}

// thread tid's block base at vector stride m (NV vectors per column)
template <int NV>
__device__ __forceinline__ int blk_base(int m) {
  const int tid = threadIdx.x;
  return (tid / m) * (m * NV) + tid % m;
}

// Compile-time form of blk_pad at vector stride M (NV outputs per column, TIGHT: blk_tight).  A
// thread's block base vb = (tid/M)*M*NV + tid%M; when M*NV is a multiple of the pad group 2^SH, the
// physical offset of logical vector vb + q*M from vb's is off(q) for every thread, so the branch
// reads at immediate offsets from one base address instead of computing u + (u >> SH)*PAD per read.
template <int M, int NV, int TIGHT>
struct BlkC {
  static constexpr int SH = blk_pad(M, NV, TIGHT).sh;
  static constexpr int PAD = blk_pad(M, NV, TIGHT).pad;
  static constexpr bool ok = PAD == 0 || (M * NV) % (1 << SH) == 0;
  static constexpr int off(int q) { return q * M + ((q * M) >> SH) * PAD; }
};

// The run-time counterpart of BlkC::off where the pad groups align with a thread's block: the physical
// offset of logical vector vb + q*m from vb's is q*m + ((q*m) >> sh)*pad for every thread -- a scalar
// value; q*m < 0 shifts arithmetically (floor), as blk_phys does.
__device__ __forceinline__ int blk_off_uniform(int qm, int sh, int pad) {
  qm = __builtin_amdgcn_readfirstlane(qm);
  return __builtin_amdgcn_readfirstlane(qm + (qm >> sh) * pad);
}

// f(integral_constant<int, m>) for a vector stride m in {1, 2, 4, .., 64} (immediate LDS offsets stay
// below 64 KiB for L <= 30); false for any other m: the caller runs its generic form.
template <typename F>
__device__ __forceinline__ bool blk_stride(int m, F&& f) {
  switch (m) {
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    case 8: f(std::integral_constant<int, 8>{}); return true;
    case 16: f(std::integral_constant<int, 16>{}); return true;
    case 32: f(std::integral_constant<int, 32>{}); return true;
    case 64: f(std::integral_constant<int, 64>{}); return true;
    default: return false;
  }
}

// Tap chunk of the blocked kernels: 8, or 4 where NV = 8 fp64 accumulators already take 32-64 VGPRs
// (1024-thread workgroups cap a lane at 128 VGPRs; 8-tap chunks spilled there).
template <typename T, int NV>
constexpr int blk_chunk() { return (NV >= 8 && sizeof(T) == 8) ? 4 : kWinTaps; }

// One branch of the inverse (reads t + i*s): acc[r] (+)= f[i] * in[vb + (r+i)m], i ascending per r;
// at(q) returns the input vector vb + q*m (an always_inline reader: the blk_inv_branch* forms below).
// Taps in chunks of blk_chunk (each re-read at its start): NV+TC-1 reads per chunk, the chunk's taps
// the only ones live.
template <typename T, int L, bool FMA, int NV, typename At>
__device__ __forceinline__ void blk_inv_taps(const At& at, const T* f, T (&acc)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  constexpr int TC = blk_chunk<T, NV>();
  static_for<0, (L + TC - 1) / TC>([&](auto c) __attribute__((always_inline)) {
    constexpr int I0 = decltype(c)::value * TC;
    constexpr int I1 = (I0 + TC < L) ? I0 + TC : L;
    T fc[I1 - I0];
#pragma unroll
    for (int i = I0; i < I1; ++i) fc[i - I0] = f[i];
#pragma unroll
    for (int q = I0; q < I1 + NV - 1; ++q) {
      const vec x = at(q);
#pragma unroll
      for (int r = 0; r < NV; ++r) {
        const int i = q - r;
        if (i >= I0 && i < I1) {
          vmadd<FMA>(acc[r], x, fc[i - I0]);
        }
      }
      if (((q - I0) & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // bounded reads in flight
    }
  });
#pragma unroll
  for (int r = 0; r < NV; ++r)
#pragma unroll
    for (int e = 0; e < V; ++e) asm volatile("" : "+v"(acc[r][e]));  // pin the sums (see inv_row_t)
}

// The forward (reads t - i*s, both filters from one set of reads): within a tap chunk q runs down so
// that for every output r the tap i = r - q ascends; chunks ascend.  at(q) returns the input vector
// vb + q*m (the blk_fwd* forms below).
template <typename T, int L, bool FMA, int NV, typename At>
__device__ __forceinline__ void blk_fwd_taps(const At& at, const T* flo, const T* fhi, T (&al)[NV][VT<T>::V],
                                             T (&ah)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  constexpr int TC = blk_chunk<T, NV>();
#pragma unroll
  for (int r = 0; r < NV; ++r)
#pragma unroll
    for (int e = 0; e < V; ++e) { al[r][e] = T(0); ah[r][e] = T(0); }
  static_for<0, (L + TC - 1) / TC>([&](auto c) __attribute__((always_inline)) {
    constexpr int I0 = decltype(c)::value * TC;
    constexpr int I1 = (I0 + TC < L) ? I0 + TC : L;
    T fl[I1 - I0], fh[I1 - I0];
#pragma unroll
    for (int i = I0; i < I1; ++i) { fl[i - I0] = flo[i]; fh[i - I0] = fhi[i]; }
#pragma unroll
    for (int q = NV - 1 - I0; q > -I1; --q) {
      const vec x = at(q);
#pragma unroll
      for (int r = 0; r < NV; ++r) {
        const int i = r - q;
        if (i >= I0 && i < I1) {
          vmadd<FMA, kPkFwd>(al[r], x, fl[i - I0]);
          vmadd<FMA, kPkFwd>(ah[r], x, fh[i - I0]);
        }
      }
      if (((NV - 1 - I0 - q) & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
  });
#pragma unroll
  for (int r = 0; r < NV; ++r)
#pragma unroll
    for (int e = 0; e < V; ++e) {
      asm volatile("" : "+v"(al[r][e]));
      asm volatile("" : "+v"(ah[r][e]));
    }
}

// The inverse branch's readers.  Per lane: blk_phys per read, any stride and layout.
template <typename T, int L, bool FMA, int NV>
__device__ __forceinline__ void blk_inv_branch(const T* R, const BlkLayout& lo, int vb, int m, const T* f,
                                               T (&acc)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  blk_inv_taps<T, L, FMA, NV>(
      [&](int q) __attribute__((always_inline)) { return blk_load(R + blk_phys(lo, vb + q * m) * V); }, f, acc);
}

// blk_inv_branch at a compile-time stride: Rb = R + blk_phys(layout, vb) * V
template <typename T, int L, bool FMA, int NV, int M, int TIGHT>
__device__ __forceinline__ void blk_inv_branch_c(const T* Rb, const T* f, T (&acc)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using C = BlkC<M, NV, TIGHT>;
  blk_inv_taps<T, L, FMA, NV>([&](int q) __attribute__((always_inline)) { return blk_load(Rb + C::off(q) * V); }, f,
                              acc);
}

// blk_inv_branch with wave-uniform offsets (blk_off_uniform, under the same condition as BlkC::ok): a
// read costs one vector add (base + scalar offset) instead of the per-lane shift / multiply / add of
// blk_phys.  One code copy for every stride (the compile-time forms, one copy per m, measured slower
// at NV = 8).
template <typename T, int L, bool FMA, int NV>
__device__ __forceinline__ void blk_inv_branch_s(const T* Rb, int m, int sh, int pad, const T* f,
                                                 T (&acc)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  blk_inv_taps<T, L, FMA, NV>(
      [&](int q) __attribute__((always_inline)) { return blk_load(Rb + blk_off_uniform(q * m, sh, pad) * V); }, f, acc);
}

// blk_inv_branch_c with the base laundered into a 32-bit LDS address (lds_base): every read is one
// ds_read_b128 at an immediate offset -- no per-read scalar offset arithmetic (blk_inv_branch_s: four SALU
// and one VALU per read) and no re-based 64-bit pointers.
template <typename T, int L, bool FMA, int NV, int M, int TIGHT>
__device__ __forceinline__ void blk_inv_branch_cl(const T* Rb, const T* f, T (&acc)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  using C = BlkC<M, NV, TIGHT>;
  const unsigned ab = lds_base(Rb);
  blk_inv_taps<T, L, FMA, NV>(
      [&](int q) __attribute__((always_inline)) {
        return lds_vec_at<vec>(ab + (unsigned)(C::off(q) * V * (int)sizeof(T)));
      },
      f, acc);
}

// One inverse branch at vector stride m >= 1: the compile-time forms for m = 1..64, the generic ones
// otherwise.  Same reads, same sums.
template <typename T, int L, bool FMA, int NV>
__device__ __forceinline__ void blk_inv_any(const T* R, const BlkLayout& lo, int tight, int vb, int m, const T* f,
                                            T (&acc)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  if constexpr (NV >= 8) {
    // compile-time forms through plain pointers measured slower at NV = 8 (sym8 fp64 inverse 7.18 -> 8.08 ms,
    // profiles/r03/ab_sym8_cinv.log); off a laundered 32-bit base (blk_inv_branch_cl) they win: 6.32-6.38
    // -> 6.17-6.28 ms (profiles/r05/ab_sym8_inverse_ck8.log; the same for k_forward_blk measured slower:
    // forward 4.92-4.97 vs 4.78-4.85 ms, sym8)
    const int sh = __builtin_amdgcn_readfirstlane(lo.sh), pad = __builtin_amdgcn_readfirstlane(lo.pad);
    if constexpr (FMA) {
      // m = 1..64 where the pad group (8 vectors, or 16 in the tight layout) divides a thread's 8m-vector
      // block (BlkC::ok) or there is none (m >= 16): the offset of vb + q*m from vb is the same for every
      // lane.  FMA only: the EXACT kernel (mul + add per tap) spills 28 B/lane at its 128-VGPR cap with it.
      const T* Rb = R + blk_phys(lo, vb) * V;
      const int sel = (m == 1 || m == 2 || m == 4 || m == 8) && pad == 1 ? m * 2 + (tight ? 1 : 0)
                      : (m == 16 || m == 32 || m == 64) && pad == 0 ? 4 * m : 0;
      switch (sel) {
        case 2: blk_inv_branch_cl<T, L, FMA, NV, 1, 0>(Rb, f, acc); return;
        // (m = 1 in the tight layout: a thread's 8-vector block is half a 16-vector pad group -- per lane)
        case 4: blk_inv_branch_cl<T, L, FMA, NV, 2, 0>(Rb, f, acc); return;
        case 5: blk_inv_branch_cl<T, L, FMA, NV, 2, 1>(Rb, f, acc); return;
        case 8: blk_inv_branch_cl<T, L, FMA, NV, 4, 0>(Rb, f, acc); return;
        case 9: blk_inv_branch_cl<T, L, FMA, NV, 4, 1>(Rb, f, acc); return;
        case 16: blk_inv_branch_cl<T, L, FMA, NV, 8, 0>(Rb, f, acc); return;
        case 17: blk_inv_branch_cl<T, L, FMA, NV, 8, 1>(Rb, f, acc); return;
        case 64: blk_inv_branch_cl<T, L, FMA, NV, 16, 0>(Rb, f, acc); return;   // m >= 16: natural layout
        case 128: blk_inv_branch_cl<T, L, FMA, NV, 32, 0>(Rb, f, acc); return;
        case 256: blk_inv_branch_cl<T, L, FMA, NV, 64, 0>(Rb, f, acc); return;
        default: break;
      }
    }
    // wave-uniform offsets where the layout allows, else per lane
    if (pad == 0 || ((m * NV) & ((1 << sh) - 1)) == 0)
      blk_inv_branch_s<T, L, FMA, NV>(R + blk_phys(lo, vb) * V, m, sh, pad, f, acc);
    else
      blk_inv_branch<T, L, FMA, NV>(R, lo, vb, m, f, acc);
  } else {
    (void)tight;  // the tight layout exists only at NV >= 8
    const T* Rb = R + blk_phys(lo, vb) * V;
    const bool ct = blk_stride(m, [&](auto mc) __attribute__((always_inline)) {
      constexpr int M = decltype(mc)::value;
      if constexpr (BlkC<M, NV, 0>::ok) blk_inv_branch_c<T, L, FMA, NV, M, 0>(Rb, f, acc);
      else blk_inv_branch<T, L, FMA, NV>(R, lo, vb, m, f, acc);
    });
    if (!ct) blk_inv_branch<T, L, FMA, NV>(R, lo, vb, m, f, acc);
  }
}

// The forward's readers; input vector u sits at logical u + HLV.  Per lane: any stride, layout and halo.
template <typename T, int L, bool FMA, int NV>
__device__ __forceinline__ void blk_fwd(const T* X, const BlkLayout& lo, int HLV, int vb, int m, const T* flo,
                                        const T* fhi, T (&al)[NV][VT<T>::V], T (&ah)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  blk_fwd_taps<T, L, FMA, NV>(
      [&](int q) __attribute__((always_inline)) { return blk_load(X + blk_phys(lo, vb + q * m + HLV) * V); }, flo, fhi,
      al, ah);
}

// blk_fwd with wave-uniform offsets (as blk_inv_branch_s): Xb = X + blk_phys(layout, vb + HLV) * V, and the
// read of logical vector vb + HLV + q*m sits blk_off_uniform(q*m) from it for every thread when the pad
// groups align with a thread's block and HLV is a multiple of the group (host: vw_plan.cpp blk_plan
// rounds HLV up to 16 vectors).
template <typename T, int L, bool FMA, int NV>
__device__ __forceinline__ void blk_fwd_s(const T* Xb, int m, int sh, int pad, const T* flo, const T* fhi,
                                          T (&al)[NV][VT<T>::V], T (&ah)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  blk_fwd_taps<T, L, FMA, NV>(
      [&](int q) __attribute__((always_inline)) { return blk_load(Xb + blk_off_uniform(q * m, sh, pad) * V); }, flo, fhi,
      al, ah);
}

// blk_fwd at a compile-time stride M (NV < 8, as blk_inv_branch_c): with the halo HLV a multiple of 16
// vectors (host) the physical offset of logical vector vb + HLV + q*M from vb + HLV's is BlkC::off(q)
// for every thread.  The reads run q = -(L-1) .. NV-1; they are addressed from the lowest one, laundered
// into a 32-bit LDS base (lds_base: through a plain pointer the compiler re-based most of them, 3 of 63 reads
// per coif5 fp32 block kept an immediate), so every offset is a non-negative immediate of the ds_read.
template <typename T, int L, bool FMA, int NV, int M>
__device__ __forceinline__ void blk_fwd_c(const T* Xb, const T* flo, const T* fhi, T (&al)[NV][VT<T>::V],
                                          T (&ah)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  using C = BlkC<M, NV, 0>;
  constexpr int QMIN = -(L - 1);
  const unsigned aq = lds_base(Xb + C::off(QMIN) * V);  // laundered: every read at an immediate offset
  blk_fwd_taps<T, L, FMA, NV>(
      [&](int q) __attribute__((always_inline)) {
        return lds_vec_at<vec>(aq + (unsigned)((C::off(q) - C::off(QMIN)) * V * (int)sizeof(T)));
      },
      flo, fhi, al, ah);
}

// One forward level at vector stride m >= 1, NV < 8: the compile-time forms for m = 1..64, the generic one
// otherwise.  Same reads, same sums (bit-identical to blk_fwd).
template <typename T, int L, bool FMA, int NV>
__device__ __forceinline__ void blk_fwd_any(const T* X, const BlkLayout& lo, int HLV, int vb, int m, const T* flo,
                                            const T* fhi, T (&al)[NV][VT<T>::V], T (&ah)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  const T* Xb = X + blk_phys(lo, vb + HLV) * V;
  const bool ct = blk_stride(m, [&](auto mc) __attribute__((always_inline)) {
    constexpr int M = decltype(mc)::value;
    if constexpr (BlkC<M, NV, 0>::ok) blk_fwd_c<T, L, FMA, NV, M>(Xb, flo, fhi, al, ah);
    else blk_fwd<T, L, FMA, NV>(X, lo, HLV, vb, m, flo, fhi, al, ah);
  });
  if (!ct) blk_fwd<T, L, FMA, NV>(X, lo, HLV, vb, m, flo, fhi, al, ah);
}

#ifndef VW_INV_KTAPS
#define VW_INV_KTAPS -1  // k_inverse_blk: taps from the kernel arguments (SGPRs) instead of LDS; -1: at NV >= 8
#endif

#ifndef VW_FWD_KTAPS
#define VW_FWD_KTAPS -1  // k_forward_blk: taps from the kernel arguments (SGPRs) instead of LDS; -1: at NV >= 8 (coif5 NV = 4: neutral)
#endif

// Forward, PERIODIC, one signal per workgroup: MultiLevelMODWTTransform.decompose (:243-251) /
// BatchSIMDMODWT.batchMultiLevelMODWTSoA (:362-377) / VectorWaveSwtAdapter forward.  Level inputs in
// one LDS buffer (p.region1 == 0: two barriers per level) or two (one barrier).  Left wrap images:
// element t is also the value at t - N.  Host contract: unrolled (L > 0), aligned rows, nvec =
// threads * NV, nvec a multiple of NV * m_J, no validation / history, p.hlpad = HLV * V.
template <typename T, int L, bool FMA, int NV>
__global__ void VW_FUSED_BOUNDS(NV, VW_FUSED_W(L, 8)) k_forward_blk(const FwdArgs<T> p) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* X = reinterpret_cast<T*>(smem);
  T* Y = p.region1 ? X + p.region1 : X;
  const bool dbl = p.region1 != 0;
  const long long b = blockIdx.x;
  // the taps live in LDS (p.tap_lds): read per level and chunk, never hoisted out of the level loop --
  // all 2L taps of a long filter held in registers across it spill (60 for coif5)
  T* const taps = reinterpret_cast<T*>(smem) + p.tap_lds;
  for (int i = threadIdx.x; i < 2 * L; i += blockDim.x) taps[i] = i < L ? p.lo[i] : p.hi[i - L];
  // kernel-argument taps (scalar loads, SGPR operands) at NV = 8 as in k_inverse_blk: fp64 L = 16 128 VGPRs
  // + 12 B/lane of scratch -> 99, none
  constexpr bool ktaps = VW_FWD_KTAPS < 0 ? NV >= 8 : VW_FWD_KTAPS != 0;
  const T* const flo = ktaps ? p.lo : taps;
  const T* const fhi = ktaps ? p.hi : taps + L;
  const int N = p.N;
  const int nvec = N / V;
  const int NT = blockDim.x;
  const int tid = threadIdx.x;
  const int HLV = p.hlpad / V;
  auto m_of = [&](int j) { return p.lv[j - 1].s / V; };
  auto hlv_of = [&](int j) { return ((L - 1) * p.lv[j - 1].s + V - 1) / V; };
  // vector w of level j's input (+ its left wrap image)
  auto put = [&](T* buf, int j, int w, const vec& o) {
    const BlkLayout lo = blk_pad(m_of(j), NV, p.blk_tight);
    blk_store<T>(buf, lo, w + HLV, o);
    if (w >= nvec - hlv_of(j)) blk_store<T>(buf, lo, w - nvec + HLV, o);
  };
  {
    T r0[NV][V];
    load_row_regs<T, NV>(r0, p.x + b * p.ldx, N, nvec, true, false);
    wait_vmem();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      int w = tid + k * NT;
      asm volatile("" : "+v"(w));
      vec o;
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] = r0[k][e];
      put(X, 1, w, o);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  T nf = T(0);  // VW_FLAG_REF_NONFINITE: a_J's probe (as k_forward_persist)
  for (int j = 1; j <= p.J; ++j) {
    const int m = m_of(j);
    lds_barrier();  // X = level input + images; every read of Y (previous level) done
    T* dout = p.details + ((size_t)(j - 1) * (size_t)p.B + (size_t)b) * (size_t)N;
    T* aout = p.approx + b * (size_t)N;
    const bool last = j == p.J;
    T al[NV][V], ah[NV][V];
    int vb = 0;
    if (m) {
      vb = blk_base<NV>(m);
      const BlkLayout lo = blk_pad(m, NV, p.blk_tight);
      if constexpr (NV < 8) {
        // compile-time stride forms where the halo is whole pad groups, else per lane
        if ((HLV & 15) == 0) blk_fwd_any<T, L, FMA, NV>(X, lo, HLV, vb, m, flo, fhi, al, ah);
        else blk_fwd<T, L, FMA, NV>(X, lo, HLV, vb, m, flo, fhi, al, ah);
      } else {
        // wave-uniform offsets where the layout allows, else per lane
        const int sh = __builtin_amdgcn_readfirstlane(lo.sh), pad = __builtin_amdgcn_readfirstlane(lo.pad);
        if (pad == 0 || (((m * NV) & ((1 << sh) - 1)) == 0 && (HLV & ((1 << sh) - 1)) == 0))
          blk_fwd_s<T, L, FMA, NV>(X + blk_phys(lo, vb + HLV) * V, m, sh, pad, flo, fhi, al, ah);
        else
          blk_fwd<T, L, FMA, NV>(X, lo, HLV, vb, m, flo, fhi, al, ah);
      }
      if (m < VW_BLK_NT_M) {
        // a lane's outputs are m*16-byte pieces NV*m*16 bytes apart: write-back stores, so that L2
        // merges a line's pieces before it goes to HBM (nontemporal stores of 16-byte pieces wrote
        // 1.5x the algorithmic bytes on coif5 fp32, profiles/hbm_traffic_coif5-f32.json)
#pragma unroll
        for (int r = 0; r < NV; ++r) {
          store_vec<0>(dout, (vb + r * m) * V, N, true, ah[r]);
          if (last) store_vec<0>(aout, (vb + r * m) * V, N, true, al[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < NV; ++r) {
          store_vec<VW_FWD_STORE_AUX>(dout, (vb + r * m) * V, N, true, ah[r]);
          if (last) store_vec<VW_FWD_STORE_AUX>(aout, (vb + r * m) * V, N, true, al[r]);
        }
      }
    } else {
      // s < V (m == 0): only the register-window forms.  (fwd_row's strided form, unreachable here,
      // kept all 2L taps of its loop live and spilled coif5 fp32: 193 VGPRs of scratch, 1.5x the
      // kernel's HBM write bytes -- profiles/r02/hbm_traffic_coif5-f32.json.)
      auto em = [&](int k, int w, const T (&l)[V], const T (&h)[V]) {
        store_vec<VW_FWD_STORE_AUX>(dout, w * V, N, true, h);
        if (last) store_vec<VW_FWD_STORE_AUX>(aout, w * V, N, true, l);
#pragma unroll
        for (int e = 0; e < V; ++e) { al[k][e] = l[e]; ah[k][e] = h[e]; }
      };
      if constexpr (V == 4) {
        if (p.lv[j - 1].s == 2) fwd_row_t<T, L, FMA, NV, 2>(X + HLV * V, nvec, 2, flo, fhi, p.taps, em);
        else fwd_row_t<T, L, FMA, NV, 1>(X + HLV * V, nvec, 1, flo, fhi, p.taps, em);
      } else {
        fwd_row_t<T, L, FMA, NV, 1>(X + HLV * V, nvec, 1, flo, fhi, p.taps, em);
      }
    }
    if (p.nf_flag && last) {
#pragma unroll
      for (int r = 0; r < NV; ++r) nf_probe<T, V>(nf, al[r]);
    }
    if (!last) {
      if (!dbl) lds_barrier();  // one buffer: every read of this level's input done first
#pragma unroll
      for (int r = 0; r < NV; ++r) {
        int w = m ? vb + r * m : tid + r * NT;
        asm volatile("" : "+v"(w));
        vec o;
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = al[r][e];
        put(Y, j + 1, w, o);
        __builtin_amdgcn_sched_barrier(0);
      }
      T* t = X; X = Y; Y = t;
    }
  }
  if (p.nf_flag) nf_flag_row<T>(p.nf_flag, b, nf);
}

// Inverse, PERIODIC, sequential sums (K4), one region time-shared as k_inverse_seq.  Right wrap
// images: element t is also the value at t + N.  Host contract as k_forward_blk (hlpad = 0).
template <typename T, int L, bool FMA, int NV>
__global__ void VW_FUSED_BOUNDS(NV, VW_FUSED_W(L, 6)) k_inverse_blk(const InvArgs<T> p) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* R = reinterpret_cast<T*>(smem);
  const long long b = p.rev ? p.B - 1 - (long long)blockIdx.x : (long long)blockIdx.x;
  const int N = p.N;
  const int nvec = N / V;
  const int NT = blockDim.x;
  const int tid = threadIdx.x;
  T* const taps = reinterpret_cast<T*>(smem) + p.tap_lds;  // as k_forward_blk
  for (int i = tid; i < 2 * L; i += NT) taps[i] = i < L ? p.lo[i] : p.hi[i - L];
  // NV = 8 (sym8 fp64 at N = 16384): the taps from the kernel arguments -- scalar loads, SGPR operands of the
  // FMAs -- free the VGPRs that held them (128 + 12-40 B/lane of scratch -> 123-125, none) and the LDS tap
  // reads: inverse 6.72-6.77 -> 6.27-6.32 ms.  NV = 4 (coif5 fp32) keeps them in LDS: there the freed VGPRs
  // admit a third workgroup per CU and the inverse slows, 6.73-6.80 -> 6.94-6.96 ms
  // (profiles/r04/ab_ktaps_coif5_sym8.log)
  constexpr bool ktaps = VW_INV_KTAPS < 0 ? NV >= 8 : VW_INV_KTAPS != 0;
  const T* const flo = ktaps ? p.lo : taps;
  const T* const fhi = ktaps ? p.hi : taps + L;
  auto thr_of = [&](int j) { return p.thr ? load_uniform(p.thr + (size_t)(j - 1) * (size_t)p.thr_ld + (size_t)b) : T(0); };
  const size_t plane = (size_t)p.B * (size_t)N;
  auto m_of = [&](int j) { return p.lv[j - 1].s / V; };
  auto hrv_of = [&](int j) { return ((L - 1) * p.lv[j - 1].s + V - 1) / V; };
  auto put = [&](int j, int w, const vec& o) {
    const BlkLayout lo = blk_pad(m_of(j), NV, p.blk_tight);
    blk_store<T>(R, lo, w, o);
    if (w < hrv_of(j)) blk_store<T>(R, lo, w + nvec, o);
  };
  // a row held in the standard mapping (w = tid + k*NT) into level j's layout; MODE as regs_to_level_m
  auto stage_std = [&](const T (&r)[NV][V], int j, int mode, T thr_b) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      int w = tid + k * NT;
      asm volatile("" : "+v"(w));
      vec o;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (mode == 1) o[e] = T(0);
        else if (mode == 2) o[e] = threshold_t(r[k][e], thr_b, p.soft);
        else o[e] = r[k][e];
      }
      put(j, w, o);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  T acc[NV][V];
  T dreg[NV][V];
  load_row_regs<T, NV>(acc, p.approx + b * (size_t)N, N, nvec, true, p.approx_zero != 0);
  load_row_regs<T, NV>(dreg, p.details + (size_t)(p.J - 1) * plane + b * (size_t)N, N, nvec, true,
                       p.lv[p.J - 1].use_d == 0);
  wait_vmem();
  stage_std(acc, p.J, p.approx_zero ? 1 : 0, T(0));

  for (int j = p.J; j >= 1; --j) {
    const LevelDesc lv = p.lv[j - 1];
    const int m = m_of(j);
    const BlkLayout lo = blk_pad(m, NV, p.blk_tight);
    const int vb = m ? blk_base<NV>(m) : 0;
    lds_barrier();  // R = a_j + wrap images
    zero_regs<T, NV>(acc);
    if (m) blk_inv_any<T, L, FMA, NV>(R, lo, p.blk_tight, vb, m, flo, acc);
    else inv_row<T, L, FMA, NV>(R, nvec, lv.s, 1, 0, flo, p.taps, 0, acc);
    lds_barrier();  // every approximation-branch read done
    wait_vmem();    // the d_j prefetch
    stage_std(dreg, j, lv.use_d == 0 ? 1 : (p.thr ? 2 : 0), thr_of(j));
    if (j > 1)
      load_row_regs<T, NV>(dreg, p.details + (size_t)(j - 2) * plane + b * (size_t)N, N, nvec, true,
                           p.lv[j - 2].use_d == 0);
    lds_barrier();  // R = d_j + wrap images
    if (m) blk_inv_any<T, L, FMA, NV>(R, lo, p.blk_tight, vb, m, fhi, acc);
    else inv_row<T, L, FMA, NV>(R, nvec, lv.s, 1, 0, fhi, p.taps, 0, acc);
    if (j > 1) {
      lds_barrier();  // every detail-branch read done
#pragma unroll
      for (int r = 0; r < NV; ++r) {
        int w = m ? vb + r * m : tid + r * NT;
        asm volatile("" : "+v"(w));
        vec o;
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = acc[r][e];
        put(j - 1, w, o);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // level 1 (s = 1 < V) ran in the standard mapping: coalesced stores
#pragma unroll
  for (int k = 0; k < NV; ++k) store_vec<VW_INV_STORE_AUX>(p.y + b * (size_t)N, (tid + k * NT) * V, N, true, acc[k]);
  if (p.nf_flag) {  // VW_FLAG_REF_NONFINITE: y's probe (as k_inverse_seq)
    T nf = T(0);
#pragma unroll
    for (int k = 0; k < NV; ++k) nf_probe<T, V>(nf, acc[k]);
    nf_flag_row<T>(p.nf_flag, b, nf);
  }
}

}  // namespace vw
