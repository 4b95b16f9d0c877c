#pragma once
// vw_dev_rows.h -- the row bodies of the fused kernels: one level's convolution over the NV vectors a thread holds
// (fwd_row* / inv_row*), on vw_dev_core.h's tap windows.  Included by the fused families (vw_dev_fwd.h,
// vw_dev_inv.h) and by the units that run a cascade of their own (vw_mra.hip, vw_energy.hip).
#include "vw_dev_core.h"

#pragma clang fp contract(off)

namespace vw {

// ---- Row compute: one level's convolution over the thread's NV vectors -------------------------
// Forward, both filters from one set of LDS reads; emit(k, w, al, ah) consumes each output vector.
// SC: 1 / 2 = register window for spacing 1 / 2 (the latter fp32 only), 0 = strided b128 reads.
template <typename T, int L, bool FMA, int NV, int SC, bool FULL = false, int LH = L, typename Emit>
__device__ __forceinline__ void fwd_row_t(const T* buf, int nvec, int s, const T* lo, const T* hi, int taps,
                                          Emit&& emit, int taps_hi = -1) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  constexpr int LM = L > LH ? L : LH;
  for_vecs<L, NV, FULL>(nvec, [&](int k, int w) {
    const int t0 = w * V;
    T al[V], ah[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { al[e] = T(0); ah[e] = T(0); }
    if constexpr (L > 0 && SC > 0) {
      fwd_window<T, L, FMA, SC, LH>(buf, t0, lo, hi, al, ah);
    } else if constexpr (L > 0) {
#pragma unroll
      for (int i = 0; i < LM; ++i) {  // s is a multiple of V: aligned 16-byte reads
        const vec v = *reinterpret_cast<const vec*>(buf + t0 - i * s);
        if (i < L) vmadd<FMA, kPkFwd>(al, v, lo[i]);
        if (i < LH) vmadd<FMA, kPkFwd>(ah, v, hi[i]);
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // <= 4 reads in flight (VGPR budget)
      }
    } else {
      fwd_vec<T, 0, FMA>(buf, t0, s, lo, hi, taps, al, ah, taps_hi);
    }
    emit(k, w, al, ah);
  });
}

// Strided levels at a COMPILE-TIME spacing S (tap-unrolled short filters): the taps' addresses differ by
// constants, so one laundered 32-bit LDS base per output vector -- the lowest address of the tap window,
// every offset non-negative and within the 16-bit field -- serves all L reads as ds_read_b128 base
// offset:imm.  With a run-time spacing each read pays its own address instruction (a v_lshl_add / v_add /
// v_subrev per tap: as much issue time as a v_fma_f64).  Same taps, same order, same arithmetic as SC = 0.
#define VW_CT_SPACINGS(X) X(2) X(4) X(8) X(16) X(32) X(64)
template <typename T, int L, bool FMA, int NV, int S, bool FULL, int LH = L, typename Emit>
__device__ __forceinline__ void fwd_row_ct(const T* buf, int nvec, const T* lo, const T* hi, Emit&& emit) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  constexpr int LM = L > LH ? L : LH;
  static_assert(S % V == 0 && (LM - 1) * S * (int)sizeof(T) < 65536, "aligned reads, 16-bit offsets");
  const T* const low = buf - (LM - 1) * S;  // the last tap, the lowest address (uniform part)
  for_vecs<L, NV, FULL>(nvec, [&](int k, int w) {
    const int t0 = w * V;
    T al[V], ah[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { al[e] = T(0); ah[e] = T(0); }
    const unsigned a0 = lds_base(low + t0);
#pragma unroll
    for (int i = 0; i < LM; ++i) {
      const vec v = lds_vec_at<vec>(a0 + (unsigned)((LM - 1 - i) * S * (int)sizeof(T)));
      if (i < L) vmadd<FMA, kPkFwd>(al, v, lo[i]);
      if (i < LH) vmadd<FMA, kPkFwd>(ah, v, hi[i]);
      // <= 4 reads in flight, as the run-time body; 8 measured the same (profiles/r07/ab_db4_level_ct.log)
      if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    emit(k, w, al, ah);
  });
}

// ct: the level's spacing is dispatched ONCE per row and level to a compile-time-stride body (VW_LEVEL_CT);
// any other spacing, and ct = 0, run the run-time-stride body.
template <typename T, int L, bool FMA, int NV, bool FULL = false, int LH = L, typename Emit>
__device__ __forceinline__ void fwd_row(const T* buf, int nvec, int s, const T* lo, const T* hi, int taps, int ct,
                                        Emit&& emit, int taps_hi = -1) {
  constexpr int V = VT<T>::V;
  if constexpr (L > 0) {
    if (s == 1) return fwd_row_t<T, L, FMA, NV, 1, FULL, LH>(buf, nvec, s, lo, hi, taps, emit);
    if constexpr (V == 4) {
      if (s == 2) return fwd_row_t<T, L, FMA, NV, 2, FULL, LH>(buf, nvec, s, lo, hi, taps, emit);
    }
  }
  if constexpr (L > 0 && L <= 8 && LH <= 8) {
    if (ct) {
      switch (s) {
#define VW_CASE(n) \
        case n:    \
          if constexpr (n % V == 0) return fwd_row_ct<T, L, FMA, NV, n, FULL, LH>(buf, nvec, lo, hi, emit); \
          break;
        VW_CT_SPACINGS(VW_CASE)
#undef VW_CASE
        default: break;
      }
    }
  }
  fwd_row_t<T, L, FMA, NV, 0, FULL, LH>(buf, nvec, s, lo, hi, taps, emit, taps_hi);
}

// Inverse, one branch over the row: acc[k]_e (+)= f[i] * buf[t0 + e + dir*i*s + off], i ascending
// (MultiLevelMODWTTransform.java:578-588 periodic, :612-639 symmetric orientations).
// SC as above; SC = -1: generic per-element form (runtime taps, or an offset that is not a
// multiple of V -- the symmetric alignment shifts).
template <typename T, int L, bool FMA, int NV, int SC, int DIR, bool FULL = false>
__device__ __forceinline__ void inv_row_t(const T* buf, int nvec, int s, int dir, int off, const T* f, int taps,
                                          T (&acc)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  for_vecs<L, NV, FULL>(nvec, [&](int k, int w) {
    const int t0 = w * V;
    if constexpr (L > 0 && SC > 0) {
      inv_window<T, L, FMA, SC, DIR>(buf, t0 + off, f, acc[k]);
    } else if constexpr (L > 0 && SC == 0) {
#pragma unroll
      for (int i = 0; i < L; ++i) {
        const vec v = *reinterpret_cast<const vec*>(buf + t0 + off + DIR * i * s);
        vmadd<FMA>(acc[k], v, f[i]);
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // <= 4 reads in flight (VGPR budget)
      }
    } else {
      inv_branch<T, L, FMA>(buf, t0, s, dir, off, f, taps, acc[k]);
    }
    // Pin the sums here: otherwise the arithmetic is sunk to the next use of acc (the other branch,
    // after a barrier) while the LDS reads stay put, and every read value is live until then.
#pragma unroll
    for (int e = 0; e < V; ++e) asm volatile("" : "+v"(acc[k][e]));
  });
}

// The strided branch at a compile-time spacing S (see fwd_row_ct): base = the lowest address of the tap
// window (tap 0 for DIR > 0, tap L-1 for DIR < 0), every read at an immediate offset.  off is a multiple of V.
template <typename T, int L, bool FMA, int NV, int S, int DIR, bool FULL>
__device__ __forceinline__ void inv_row_ct(const T* buf, int nvec, int off, const T* f, T (&acc)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  static_assert(S % V == 0 && (L - 1) * S * (int)sizeof(T) < 65536, "aligned reads, 16-bit offsets");
  const T* const low = buf + off - (DIR > 0 ? 0 : (L - 1) * S);  // uniform part
  for_vecs<L, NV, FULL>(nvec, [&](int k, int w) {
    const int t0 = w * V;
    const unsigned a0 = lds_base(low + t0);
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const vec v = lds_vec_at<vec>(a0 + (unsigned)((DIR > 0 ? i : L - 1 - i) * S * (int)sizeof(T)));
      vmadd<FMA>(acc[k], v, f[i]);
      if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // <= 4 reads in flight (VGPR budget)
    }
#pragma unroll
    for (int e = 0; e < V; ++e) asm volatile("" : "+v"(acc[k][e]));  // pin the sums here (see inv_row_t)
  });
}

// ct: as fwd_row -- the spacing (and direction) dispatched once per row, level and branch.
template <typename T, int L, bool FMA, int NV, bool FULL = false>
__device__ __forceinline__ void inv_row(const T* buf, int nvec, int s, int dir, int off, const T* f, int taps, int ct,
                                        T (&acc)[NV][VT<T>::V]) {
  constexpr int V = VT<T>::V;
  if constexpr (L > 0) {
    if ((off & (V - 1)) == 0) {
      if (s == 1) {
        if (dir > 0) return inv_row_t<T, L, FMA, NV, 1, 1, FULL>(buf, nvec, s, dir, off, f, taps, acc);
        return inv_row_t<T, L, FMA, NV, 1, -1, FULL>(buf, nvec, s, dir, off, f, taps, acc);
      }
      if constexpr (V == 4) {
        if (s == 2) {
          if (dir > 0) return inv_row_t<T, L, FMA, NV, 2, 1, FULL>(buf, nvec, s, dir, off, f, taps, acc);
          return inv_row_t<T, L, FMA, NV, 2, -1, FULL>(buf, nvec, s, dir, off, f, taps, acc);
        }
      }
      if constexpr (L <= 8) {
        if (ct) {
          switch (s) {
#define VW_CASE(n)                                                                                  \
            case n:                                                                                 \
              if constexpr (n % V == 0) {                                                           \
                if (dir > 0) return inv_row_ct<T, L, FMA, NV, n, 1, FULL>(buf, nvec, off, f, acc);  \
                return inv_row_ct<T, L, FMA, NV, n, -1, FULL>(buf, nvec, off, f, acc);              \
              }                                                                                     \
              break;
            VW_CT_SPACINGS(VW_CASE)
#undef VW_CASE
            default: break;
          }
        }
      }
      if (dir > 0) return inv_row_t<T, L, FMA, NV, 0, 1, FULL>(buf, nvec, s, dir, off, f, taps, acc);
      return inv_row_t<T, L, FMA, NV, 0, -1, FULL>(buf, nvec, s, dir, off, f, taps, acc);
    }
  }
  inv_row_t<T, L, FMA, NV, -1, 1, FULL>(buf, nvec, s, dir, off, f, taps, acc);
}
}  // namespace vw
