#pragma once
// vw_dev_inv.h -- the fused inverse family: k_inverse_fused (pairwise sums), k_inverse_db and k_inverse_seq
// (sequential sums, two LDS buffers / one) and the PLAIN pieces of k_inverse_seq's full-slab form.
// Launched by vw_inv.hip; vw_pair.hip's k_roundtrip runs the PLAIN pieces as its inverse half.
#include "vw_dev_rows.h"

#pragma clang fp contract(off)

namespace vw {

// ---------------------------------------------------------------------------------------------
// Fused multi-level inverse: MultiLevelMODWTTransform.reconstruct (:339-349, :554-645),
// VectorWaveSwtAdapter.reconstructPeriodic (:444-474), MODWTTransform.inverse (J=1, pairwise),
// with the denoise threshold (MutableMultiLevelMODWTResult.java:97-114) fused into the detail load.
//
// Pairwise form (sum += h*a + g*d per tap): a_j and d_j in two LDS regions.
template <typename T, int L, bool FMA, int NV>
__global__ void VW_FUSED_BOUNDS(NV, VW_FUSED_W(L, 6)) k_inverse_fused(const InvArgs<T> p) {
  constexpr int V = VT<T>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* A = reinterpret_cast<T*>(smem) + p.hlpad_a;
  T* D = reinterpret_cast<T*>(smem) + p.region_d + p.hlpad_d;
  const long long b = p.rev ? p.B - 1 - (long long)blockIdx.x : (long long)blockIdx.x;
  const int N = p.N;
  const int nvec = (N + V - 1) / V;
  const bool vec_ok = (L > 0) || p.vec_io != 0;
  // threshold of level j (denoise): thr[(j-1)*thr_ld + b]; thr_ld = 0 -> one threshold for every level
  auto thr_of = [&](int j) { return p.thr ? load_uniform(p.thr + (size_t)(j - 1) * (size_t)p.thr_ld + (size_t)b) : T(0); };
  const size_t plane = (size_t)p.B * (size_t)N;

  T reg[NV][V];
  T dnext[NV][V];
  // coarsest level: approximation -> A, d_J -> D
  load_row_regs<T, NV>(reg, p.approx + b * (size_t)N, N, nvec, vec_ok, p.approx_zero != 0);
  load_row_regs<T, NV>(dnext, p.details + (size_t)(p.J - 1) * plane + b * (size_t)N, N, nvec, vec_ok,
                       p.lv[p.J - 1].use_d == 0);
  wait_vmem();
  regs_to_level<T, L, NV>(A, reg, nvec, N, p.lv[p.J - 1], 0, (const T*)nullptr, p.approx_zero != 0);
  regs_to_level<T, L, NV>(D, dnext, nvec, N, p.lv[p.J - 1], 0, (const T*)nullptr, p.lv[p.J - 1].use_d == 0, p.thr,
                          thr_of(p.J), p.soft);

  for (int j = p.J; j >= 1; --j) {
    const LevelDesc lv = p.lv[j - 1];
    lds_barrier();  // A (level-j approximation) and D (d_j) complete, halos included
    if (j > 1) {    // prefetch d_{j-1} while this level computes
      load_row_regs<T, NV>(dnext, p.details + (size_t)(j - 2) * plane + b * (size_t)N, N, nvec, vec_ok,
                           p.lv[j - 2].use_d == 0);
    }
    for_vecs<L, NV>(nvec, [&](int k, int w) {
      T acc[V];
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = T(0);
      inv_pair<T, L, FMA>(A, D, w * V, lv.s, lv.dir_a, p.lo, p.hi, p.taps, acc);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        asm volatile("" : "+v"(acc[e]));  // pin the sum here (see inv_row_t)
        reg[k][e] = acc[e];
      }
    });
    if (j == 1) {
      for_vecs<L, NV>(nvec, [&](int k, int w) { store_vec<VW_INV_STORE_AUX>(p.y + b * (size_t)N, w * V, N, vec_ok, reg[k]); });
    } else {
      const LevelDesc ln = p.lv[j - 2];
      lds_barrier();  // all reads of A and D done
      regs_to_level<T, L, NV>(A, reg, nvec, N, ln, 0, (const T*)nullptr);
      wait_vmem();  // the d_{j-1} prefetch
      regs_to_level<T, L, NV>(D, dnext, nvec, N, ln, 0, (const T*)nullptr, ln.use_d == 0, p.thr, thr_of(j - 1), p.soft);
    }
  }
}

// Sequential-sum form (PERIODIC K4 / SYMMETRIC K6: all approximation taps, then all detail taps,
// into one accumulator), double-buffered: X holds a_j, Y holds d_j.  Per level:
//   barrier -> stage d_j (prefetched last level) into Y, prefetch d_{j-1} -> approx branch on X
//   -> barrier -> detail branch on Y -> a_{j-1} into X
// i.e. two workgroup barriers per level, and d_{j-1}'s loads have a whole level to land.
// LH: the detail branch's compile-time tap count (two-length banks, VW_BI): each branch issues its own filter's
// LDS reads and multiplies; LH = L is the equal-length kernel.
template <typename T, int L, bool FMA, int NV, int LH = L>
__global__ void VW_FUSED_BOUNDS(NV, VW_FUSED_W((L > LH ? L : LH), 6)) k_inverse_db(const InvArgs<T> p) {
  constexpr int V = VT<T>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* const X = reinterpret_cast<T*>(smem) + p.hlpad_a;
  T* const Y = reinterpret_cast<T*>(smem) + p.region_d + p.hlpad_d;
  const long long b = p.rev ? p.B - 1 - (long long)blockIdx.x : (long long)blockIdx.x;
  const int N = p.N;
  const int nvec = (N + V - 1) / V;
  const bool vec_ok = (L > 0) || p.vec_io != 0;
  // threshold of level j (denoise): thr[(j-1)*thr_ld + b]; thr_ld = 0 -> one threshold for every level
  auto thr_of = [&](int j) { return p.thr ? load_uniform(p.thr + (size_t)(j - 1) * (size_t)p.thr_ld + (size_t)b) : T(0); };
  const size_t plane = (size_t)p.B * (size_t)N;

  T acc[NV][V];
  T dreg[NV][V];
  load_row_regs<T, NV>(acc, p.approx + b * (size_t)N, N, nvec, vec_ok, p.approx_zero != 0);
  load_row_regs<T, NV>(dreg, p.details + (size_t)(p.J - 1) * plane + b * (size_t)N, N, nvec, vec_ok,
                       p.lv[p.J - 1].use_d == 0);
  wait_vmem();
  regs_to_level<T, L, NV>(X, acc, nvec, N, p.lv[p.J - 1], 0, (const T*)nullptr, p.approx_zero != 0);

  for (int j = p.J; j >= 1; --j) {
    const LevelDesc lv = p.lv[j - 1];
    lds_barrier();  // X = a_j + halo; every read of Y (previous level) done
    wait_vmem();    // the d_j prefetch (the only global ops in flight)
    regs_to_level<T, L, NV>(Y, dreg, nvec, N, lv, 0, (const T*)nullptr, lv.use_d == 0, p.thr, thr_of(j), p.soft);
    if (j > 1)
      load_row_regs<T, NV>(dreg, p.details + (size_t)(j - 2) * plane + b * (size_t)N, N, nvec, vec_ok,
                           p.lv[j - 2].use_d == 0);
    zero_regs<T, NV>(acc);
    inv_row<T, L, FMA, NV>(X, nvec, lv.s, lv.dir_a, lv.off_a, p.lo, p.taps, p.level_ct, acc);
    lds_barrier();  // Y = d_j + halo; every read of X done
    inv_row<T, LH, FMA, NV>(Y, nvec, lv.s, lv.dir_d, lv.off_d, p.hi, p.taps_hi, p.level_ct, acc);
    if (j > 1) regs_to_level<T, L, NV>(X, acc, nvec, N, p.lv[j - 2], 0, (const T*)nullptr);
  }
  for_vecs<L, NV>(nvec, [&](int k, int w) { store_vec<VW_INV_STORE_AUX>(p.y + b * (size_t)N, w * V, N, vec_ok, acc[k]); });
}

// Single-buffer sequential-sum form for signals too long for two LDS buffers: ONE region is
// time-shared (a_j -> approx branch -> d_j -> detail branch -> a_{j-1}); four barriers per level.
#ifndef VW_INV_W
#define VW_INV_W 6  // waves per SIMD of k_inverse_seq's general forms (the PLAIN form names its own: W below)
#endif
// ---- PLAIN form of the full-slab kernel -----------------------------------------------------------
// A PERIODIC reconstruction from all of its coefficients (host: InvArgs::plain): every level reads t + i*s, so
// there is no left halo and the right one is the row's first hr elements again; no threshold, no zeroed
// level, no probe, forward walk.  What the general form carries for those cases -- the level descriptor, the
// threshold pointer and stride, the modulo of the generic halo fill, 64-bit flat addresses per lane and
// vector -- is never live here, and that is what lets the kernel fit 64 VGPRs (four 512-thread workgroups
// per CU) without scratch.  The one per-lane address is the byte offset vb = (tid + k * NT) * 16 of a vector
// in its row, the same for global rows (raw buffer instructions: the row base is an SGPR resource) and LDS.
// Per output: the same LDS values, taps ascending, approximation branch then detail branch, the same
// multiply / add instructions as the general form -- bit-identical results.
template <int NV, typename F>
__device__ __forceinline__ void plain_vecs(unsigned slab, F&& fn) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    unsigned vb = threadIdx.x * 16u;
    asm volatile("" : "+v"(vb));  // only tid * 16 stays live across the level loop (see for_vecs)
    fn(k, vb + k * slab);
    __builtin_amdgcn_sched_barrier(0);  // one vector's LDS reads at a time (see for_vecs)
  }
}

// Row <-> registers; non-temporal (aux 2), as the general form's flat loads and stores.
template <typename T, int NV>
__device__ __forceinline__ void plain_load_row(T (&r)[NV][VT<T>::V], const T* row, unsigned slab) {
  using vec = typename VT<T>::v;
  const __amdgpu_buffer_rsrc_t rs = row_rsrc(row);
  unsigned vb = threadIdx.x * 16u;
  asm volatile("" : "+v"(vb));
#pragma unroll
  for (int k = 0; k < NV; ++k) {  // loads only: first touched where they are written to LDS (load_row_regs)
    const vec v = __builtin_bit_cast(vec, __builtin_amdgcn_raw_buffer_load_b128(rs, vb, k * slab, 2));
#pragma unroll
    for (int e = 0; e < VT<T>::V; ++e) r[k][e] = v[e];
  }
}
template <typename T, int NV>
__device__ __forceinline__ void plain_store_row(T* row, const T (&r)[NV][VT<T>::V], unsigned slab) {
  using vec = typename VT<T>::v;
  const __amdgpu_buffer_rsrc_t rs = row_rsrc(row);
  unsigned vb = threadIdx.x * 16u;
  asm volatile("" : "+v"(vb));
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    vec o;
#pragma unroll
    for (int e = 0; e < VT<T>::V; ++e) o[e] = r[k][e];
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(vw_i4, o), rs, vb, k * slab, 2);
  }
}

// Registers -> LDS level buffer with its right halo [N, N + hr): by the owners of elements [0, hr) where they
// all sit in the first slab (own; regs_to_level_m), else copied after a barrier (hr <= N: host contract).
template <typename T, int NV>
__device__ __forceinline__ void plain_to_level(T* R, const T (&r)[NV][VT<T>::V], unsigned slab, int N, int hr, int own) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  plain_vecs<NV>(slab, [&](int k, unsigned vb) {
    vec o;
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = r[k][e];
    T* const at = reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(R) + vb);
    *reinterpret_cast<vec*>(at) = o;
    if (k == 0 && own && vb < (unsigned)hr * (unsigned)sizeof(T)) {
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (vb + e * (unsigned)sizeof(T) < (unsigned)hr * (unsigned)sizeof(T)) at[N + e] = o[e];
    }
  });
  if (!own) {
    lds_barrier();
    for (int q = threadIdx.x; q < hr; q += blockDim.x) R[N + q] = R[q];
  }
}

// One branch over the row: acc[k]_e (+)= f[i] * R[t0 + e + i*s], i ascending (inv_row_t / inv_row_ct at
// dir = +1, off = 0).  S > 0: compile-time spacing, one base and immediate offsets; S = 0: run-time spacing;
// S < 0: the register window of spacing -S (below the vector width).  RIF: LDS reads in flight per vector.
template <typename T, int L, bool FMA, int NV, int RIF, int S>
__device__ __forceinline__ void plain_row_s(const T* R, unsigned slab, int s, const T* f, T (&acc)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  plain_vecs<NV>(slab, [&](int k, unsigned vb) {
    const T* const at = reinterpret_cast<const T*>(reinterpret_cast<const unsigned char*>(R) + vb);
    if constexpr (S < 0) {
      inv_window<T, L, FMA, -S, 1>(at, 0, f, acc[k]);
    } else {
      const unsigned a0 = lds_base(at);
#pragma unroll
      for (int i = 0; i < L; ++i) {
        const vec v = S > 0 ? lds_vec_at<vec>(a0 + (unsigned)(i * S * (int)sizeof(T)))
                            : *reinterpret_cast<const vec*>(at + i * s);
        vmadd<FMA>(acc[k], v, f[i]);
        if (i % RIF == RIF - 1) __builtin_amdgcn_sched_barrier(0);  // <= RIF reads in flight (VGPR budget)
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) asm volatile("" : "+v"(acc[k][e]));  // pin the sums here (see inv_row_t)
  });
}
template <typename T, int L, bool FMA, int NV, int RIF>
__device__ __forceinline__ void plain_row(const T* R, unsigned slab, int s, const T* f, T (&acc)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  if (s == 1) return plain_row_s<T, L, FMA, NV, RIF, -1>(R, slab, s, f, acc);
  if constexpr (V == 4) {
    if (s == 2) return plain_row_s<T, L, FMA, NV, RIF, -2>(R, slab, s, f, acc);
  }
  switch (s) {  // the spacing dispatched once per row, level and branch (inv_row)
#define VW_CASE(n)                                                                             \
    case n:                                                                                    \
      if constexpr (n % V == 0) return plain_row_s<T, L, FMA, NV, RIF, n>(R, slab, s, f, acc); \
      break;
    VW_CT_SPACINGS(VW_CASE)
#undef VW_CASE
    default: break;
  }
  plain_row_s<T, L, FMA, NV, RIF, 0>(R, slab, s, f, acc);
}

// k_inverse_seq's schedule (below), phase for phase; a level reads only its spacing, right halo and owner flag.
// W = 8 keeps three LDS reads in flight per output vector where the general form and W = 6 keep four: with
// the detail-row prefetch (16 VGPRs) and both sums live that is what 64 VGPRs hold.
template <typename T, int L, bool FMA, int NV, int W>
__device__ __forceinline__ void inverse_seq_plain(const InvArgs<T>& p) {
  constexpr int V = VT<T>::V;
  constexpr int RIF = W >= 8 ? 3 : 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* const R = reinterpret_cast<T*>(smem) + p.hlpad_a;
  const size_t N = (size_t)p.N;
  const size_t row = (size_t)blockIdx.x * N, plane = (size_t)p.B * N;
  const unsigned slab = blockDim.x * 16u;  // bytes between a lane's vectors

  T acc[NV][V];
  T dreg[NV][V];
  plain_load_row<T, NV>(acc, p.approx + row, slab);
  plain_load_row<T, NV>(dreg, p.details + (size_t)(p.J - 1) * plane + row, slab);
  wait_vmem();
  plain_to_level<T, NV>(R, acc, slab, p.N, p.lv[p.J - 1].hr, p.lv[p.J - 1].own);

  for (int j = p.J; j >= 1; --j) {
    const int s = p.lv[j - 1].s;
    lds_barrier();  // R = a_j + halo
    zero_regs<T, NV>(acc);
    plain_row<T, L, FMA, NV, RIF>(R, slab, s, p.lo, acc);
    lds_barrier();  // every approximation-branch read done
    wait_vmem();    // the d_j prefetch
    plain_to_level<T, NV>(R, dreg, slab, p.N, p.lv[j - 1].hr, p.lv[j - 1].own);
    if (j > 1)  // the d_{j-1} prefetch, in flight across the detail branch
      plain_load_row<T, NV>(dreg, p.details + (size_t)(j - 2) * plane + row, slab);
    lds_barrier();  // R = d_j + halo
    plain_row<T, L, FMA, NV, RIF>(R, slab, s, p.hi, acc);
    if (j > 1) {
      lds_barrier();  // every detail-branch read done
      plain_to_level<T, NV>(R, acc, slab, p.N, p.lv[j - 2].hr, p.lv[j - 2].own);
    }
  }
  plain_store_row<T, NV>(p.y + row, acc, slab);
}

// FULL: aligned rows with every slab full (threads * NV == N / V; host: InvArgs::full) -- the bounds
// checks of the row transfers and the ragged-row store path are compiled out (VW_LEVEL_CT).
// LH: as k_inverse_db.
// W: waves per SIMD the kernel is compiled for (VW_FUSED_BOUNDS).  PLAIN (a FULL form of the short filters):
// inverse_seq_plain at W = 6 or 8 (host: InvArgs::plain, VW_INV_WAVES).
template <typename T, int L, bool FMA, int NV, bool FULL = false, int LH = L, int W = VW_INV_W, bool PLAIN = false>
__global__ void VW_FUSED_BOUNDS(NV, VW_FUSED_W((L > LH ? L : LH), W)) k_inverse_seq(const InvArgs<T> p) {
  if constexpr (PLAIN) {
    static_assert(FULL && L > 0 && L <= 8 && LH == L && NV == 4, "the plain form is a full-slab form of the short filters");
    inverse_seq_plain<T, L, FMA, NV, W>(p);
    return;
  }
  constexpr int V = VT<T>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* R = reinterpret_cast<T*>(smem) + p.hlpad_a;
  const long long b = p.rev ? p.B - 1 - (long long)blockIdx.x : (long long)blockIdx.x;
  const int N = p.N;
  const int nvec = (N + V - 1) / V;
  const bool vec_ok = (L > 0) || p.vec_io != 0;
  // threshold of level j (denoise): thr[(j-1)*thr_ld + b]; thr_ld = 0 -> one threshold for every level
  auto thr_of = [&](int j) { return p.thr ? load_uniform(p.thr + (size_t)(j - 1) * (size_t)p.thr_ld + (size_t)b) : T(0); };
  const size_t plane = (size_t)p.B * (size_t)N;

  T acc[NV][V];
  T dreg[NV][V];
  // VW_FLAG_REF_NONFINITE: probing y flags every row vw_ref.hip must recompute (see there)
  T nf = T(0);
  const bool nfp = p.nf_flag != nullptr;
  load_row_regs<T, NV, FULL>(acc, p.approx + b * (size_t)N, N, nvec, vec_ok, p.approx_zero != 0);
  load_row_regs<T, NV, FULL>(dreg, p.details + (size_t)(p.J - 1) * plane + b * (size_t)N, N, nvec, vec_ok,
                       p.lv[p.J - 1].use_d == 0);
  wait_vmem();
  regs_to_level<T, L, NV, FULL>(R, acc, nvec, N, p.lv[p.J - 1], 0, (const T*)nullptr, p.approx_zero != 0);

  for (int j = p.J; j >= 1; --j) {
    const LevelDesc lv = p.lv[j - 1];
    lds_barrier();  // R = a_j + halo
    zero_regs<T, NV>(acc);
    inv_row<T, L, FMA, NV, FULL>(R, nvec, lv.s, lv.dir_a, lv.off_a, p.lo, p.taps, p.level_ct, acc);
    lds_barrier();  // every approximation-branch read done
    wait_vmem();    // the d_j prefetch
    regs_to_level<T, L, NV, FULL>(R, dreg, nvec, N, lv, 0, (const T*)nullptr, lv.use_d == 0, p.thr, thr_of(j), p.soft);
    if (j > 1)  // the d_{j-1} prefetch, in flight across the detail branch
      load_row_regs<T, NV, FULL>(dreg, p.details + (size_t)(j - 2) * plane + b * (size_t)N, N, nvec, vec_ok,
                           p.lv[j - 2].use_d == 0);
    lds_barrier();  // R = d_j + halo
    inv_row<T, LH, FMA, NV, FULL>(R, nvec, lv.s, lv.dir_d, lv.off_d, p.hi, p.taps_hi, p.level_ct, acc);
    if (j > 1) {
      lds_barrier();  // every detail-branch read done
      regs_to_level<T, L, NV, FULL>(R, acc, nvec, N, p.lv[j - 2], 0, (const T*)nullptr);
    }
  }
  for_vecs<L, NV, FULL>(nvec, [&](int k, int w) { store_vec<VW_INV_STORE_AUX, FULL>(p.y + b * (size_t)N, w * V, N, vec_ok, acc[k]); });
  if (nfp) {
    nf_probe_rows<T, L, NV, V, FULL>(nf, acc, nvec);
    nf_flag_row<T>(p.nf_flag, b, nf);
  }
}
}  // namespace vw
