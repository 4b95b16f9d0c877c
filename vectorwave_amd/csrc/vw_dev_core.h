#pragma once
// vw_dev_core.h -- what every hand-written CDNA4 (gfx950) HIP kernel of VectorWave's MODWT / SWT hot path shares:
// VT, madd / vmadd, the LDS and wait helpers, the halo fill, the tap windows, for_vecs, the store and load
// policies, the row transfers, the fused kernels' launch bounds and the non-finite probe.  The kernels live in the
// family headers on top of it: vw_dev_rows.h (row bodies), vw_dev_fwd.h, vw_dev_inv.h, vw_blk.h, vw_dev_lvl.h.
//
// The hot loop of the reference is the a-trous convolution of one level:
//   forward  (K1-K3)  out[t] = sum_{l=0}^{L_j-1} f_j[l] * x[g(t - l)]           ScalarOps.java:700-835
//   inverse  (K4-K6)  y[t]   = sum_l h_j[l] * a[g(t +/- l - tau)] (+) sum_l g_j[l] * d[...]
//                                                                  MultiLevelMODWTTransform.java:554-645
// with f_j the base taps * 1/sqrt(2) upsampled by 2^(j-1) (ScalarOps.java:909-916).  Only the L
// non-zero taps at spacing s = 2^(j-1) contribute; the zero taps add +/-0.0 to a sum that is never
// -0.0, so skipping them is exact.
//
// MI355X design:
//  * One workgroup per signal.  The whole level input lives in LDS with its boundary "halo"
//    materialised around it, so the inner loop is boundary-agnostic: the reference's index map g
//    (periodic wrap, zero padding, half-sample mirror, FFT zero-pad, streaming history) is applied
//    once per level when the halo is filled, not once per tap.
//  * The J-level cascade is fused: x is read from HBM once, each detail level is written once,
//    the running approximation never leaves LDS / VGPRs (forward); the inverse reads each detail
//    level once (prefetched into VGPRs while the previous level computes) and writes y once.
//  * Each lane owns 16-byte vectors of consecutive outputs (2 x fp64 / 4 x fp32): global loads
//    and stores are dwordx4 and fully coalesced; LDS reads are ds_read_b128 at spacing s, or one
//    register window for s < vector width (level 1), conflict-free (consecutive lanes, consecutive
//    16-byte slots).
//  * EXACT variant: separate v_mul_f64 / v_add_f64 in the reference's tap order (file compiled with
//    -ffp-contract=off): bit-identical to vectorwave-core.  FMA variant: v_fma_f64, ~1 ulp/tap.
//  * Bandwidth-bound stencil: no MFMA.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include "vw_internal.h"

#pragma clang fp contract(off)

namespace vw {

template <typename T> struct VT;
template <> struct VT<double> { typedef double v __attribute__((ext_vector_type(2))); static constexpr int V = 2; };
template <> struct VT<float>  { typedef float  v __attribute__((ext_vector_type(4))); static constexpr int V = 4; };

__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// acc + x*f : EXACT = rounded product then rounded sum (Java semantics); FMA = one rounding.
template <bool FMA, typename T>
__device__ __forceinline__ T madd(T acc, T x, T f) {
  if constexpr (FMA) return fma_t(x, f, acc);
  else return acc + x * f;
}

// acc_e (+)= x_e * f over one 16-byte vector of outputs, per element.  PK (fp32 only): two packed
// operations per pair (v_pk_fma_f32; EXACT v_pk_mul_f32 + v_pk_add_f32, the same rounding per
// element).  Measured on coif5 fp32, same box (profiles/r03/ab_coif5_pk_cinv.log): packed forward
// 6.46 -> 5.88 ms; packed inverse 7.05 -> 7.23 ms.  So the forward kernels pack (VW_PK_F32_FWD,
// default 1) and the inverse ones do not (VW_PK_F32, default 0).  tools/valubench.hip: v_fma_f32
// issues 95 TFLOP/s, v_pk_fma_f32 117 on this GPU.
#ifndef VW_PK_F32
#define VW_PK_F32 0
#endif
#ifndef VW_PK_F32_FWD
#define VW_PK_F32_FWD 1
#endif
constexpr bool kPkFwd = VW_PK_F32_FWD != 0;
template <bool FMA, bool PK = (VW_PK_F32 != 0), typename T, typename X>
__device__ __forceinline__ void vmadd(T* acc, const X& x, T f) {
  if constexpr (PK && std::is_same<T, float>::value) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 fv = {f, f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f2 a = {acc[2 * h], acc[2 * h + 1]};
      const f2 xv = {x[2 * h], x[2 * h + 1]};
      if constexpr (FMA) a = __builtin_elementwise_fma(xv, fv, a);
      else a = a + xv * fv;
      acc[2 * h] = a[0];
      acc[2 * h + 1] = a[1];
    }
  } else {
#pragma unroll
    for (int e = 0; e < VT<T>::V; ++e) acc[e] = madd<FMA>(acc[e], x[e], f);
  }
}

// Workgroup-uniform read of data written before the launch (thresholds, per-signal constants)
// through the constant address space: a scalar (SMEM) load.  A vector load of it inside a level loop
// would make the waitcnt pass, which cannot count across the loop's conditional load, wait vmcnt(0)
// at the loop head -- i.e. for the detail-row prefetch that is meant to stay in flight.
template <typename T>
__device__ __forceinline__ T load_uniform(const T* q) {
  typedef const __attribute__((address_space(4))) T* cptr;
  return *(cptr)(q);
}

__device__ __forceinline__ bool finite_t(double v) { return __builtin_isfinite(v); }
__device__ __forceinline__ bool finite_t(float v) { return __builtin_isfinite(v); }

// MathUtils.symmetricBoundaryExtension  core/util/MathUtils.java:30-51
__device__ __forceinline__ int sym_index(int idx, int n) {
  if (idx >= 0 && idx < n) return idx;
  int period = 2 * n;
  idx = ((idx % period) + period) % period;
  if (idx >= n) idx = period - idx - 1;
  return idx;
}

// Workgroup barrier that orders LDS only: waits for this wave's LDS operations (lgkmcnt(0)) and
// lets global stores and prefetch loads stay in flight across it.  (__syncthreads() also waits
// vmcnt(0), which would expose the latency of every detail-level store at every level.)  Values
// loaded from global memory are waited for by the compiler at their first use, as usual.
// 16-byte LDS read at a 32-bit LDS byte address.  With the base laundered (lds_base) the compiler keeps
// base + constant as ONE ds_read with the constant in its offset field, instead of re-basing on the
// highest address of a run of reads and paying a v_add per read.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wint-to-pointer-cast"
template <typename vec>
__device__ __forceinline__ vec lds_vec_at(unsigned a) {
  return *(const __attribute__((address_space(3))) vec*)a;
}
#pragma clang diagnostic pop
template <typename T>
__device__ __forceinline__ unsigned lds_base(const T* p) {
  unsigned a = (unsigned)(uintptr_t)p;
  asm volatile("" : "+v"(a));
  return a;
}

__device__ __forceinline__ void lds_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0); vmcnt / expcnt untouched
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Wait for this wave's outstanding global loads (and stores) explicitly.  Used where every
// outstanding op is one we need anyway: the waitcnt pass models exec-masked (skippable) blocks
// conservatively, and without this it keeps the prologue loads "pending" into the level loop, where
// it then waits for the detail stores of the previous level before touching those registers.
__device__ __forceinline__ void wait_vmem() { __builtin_amdgcn_s_waitcnt(0x0F70); }  // vmcnt(0)

// Value of a level input at signal index idx outside [0, N), read from the LDS copy `buf`
// (element 0 at buf[0]).  The reference's index maps; see HaloMode.
template <typename T>
__device__ __forceinline__ T halo_value_lds(const T* buf, int idx, int N, int mode, int npow2,
                                            const T* hist_b, int hist_len) {
  switch (mode) {
    case kHaloPeriodic: { int r = idx % N; if (r < 0) r += N; return buf[r]; }
    case kHaloSymmetric: return buf[sym_index(idx, N)];
    case kHaloFftPad: { int r = idx < 0 ? idx + npow2 : idx; return (r >= 0 && r < N) ? buf[r] : T(0); }
    case kHaloHistory: return (idx < 0 && idx >= -hist_len) ? hist_b[hist_len + idx] : T(0);
    default: return T(0);
  }
}

// Fill positions [-hl, 0) and [N, N+hr) of the LDS level buffer.  The streaming-history fill is a
// separate loop: it is the only global load inside the level loop, and vmcnt is in order (stores
// count too), so waiting for it would also wait for every detail store still in flight.
template <typename T>
__device__ __forceinline__ void fill_halo(T* buf, int N, int hl, int hr, int mode, int npow2,
                                          const T* hist_b, int hist_len) {
  const int total = hl + hr;
  if (mode == kHaloHistory) {
    for (int q = threadIdx.x; q < total; q += blockDim.x) {
      const int idx = q < hl ? q - hl : N + (q - hl);
      buf[idx] = (idx < 0 && idx >= -hist_len) ? hist_b[hist_len + idx] : T(0);
    }
    return;
  }
  for (int q = threadIdx.x; q < total; q += blockDim.x) {
    const int idx = q < hl ? q - hl : N + (q - hl);
    buf[idx] = halo_value_lds(buf, idx, N, mode, npow2, (const T*)nullptr, 0);
  }
}

// ---------------------------------------------------------------------------------------------
// Register windows of the levels whose spacing is below the vector width.  Long filters take their
// taps in chunks of kWinTaps, each with its own aligned sub-window (a whole-filter window of coif5
// at spacing 2 in fp32 would be 64 registers); per output the taps still ascend.
constexpr int kWinTaps = 8;

__host__ __device__ constexpr int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

template <int C, int NC, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (C < NC) {
    f(std::integral_constant<int, C>{});
    static_for<C + 1, NC>(f);
  }
}

// Forward: one 16-byte vector of consecutive outputs t0..t0+V-1, both filters from one set of
// LDS reads.  acc_e (+)= x[t0 + e - i*s] * f[i], i ascending (ScalarOps.java:707-719 order).
// LH: the high-pass tap count of a two-length bank (VW_BI): tap position i feeds the low sum only while i < L and
// the high sum only while i < LH (compile-time after unrolling: the short filter spends nothing on absent taps).
template <typename T, int L, bool FMA, int S, int LH = L>
__device__ __forceinline__ void fwd_window(const T* buf, int t0, const T* lo, const T* hi,
                                           T (&al)[VT<T>::V], T (&ah)[VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  constexpr int LM = L > LH ? L : LH;
  static_for<0, (LM + kWinTaps - 1) / kWinTaps>([&](auto c) __attribute__((always_inline)) {
    constexpr int I0 = decltype(c)::value * kWinTaps;
    constexpr int I1 = (I0 + kWinTaps < LM) ? I0 + kWinTaps : LM;
    constexpr int A = floor_div(-(I1 - 1) * S, V) * V;       // offsets e - i*S, aligned down
    constexpr int E = (floor_div(V - 1 - I0 * S, V) + 1) * V;
    constexpr int NE = E - A;
    T w[NE];
#pragma unroll
    for (int k = 0; k < NE / V; ++k) {
      vec v = *reinterpret_cast<const vec*>(buf + t0 + A + k * V);
#pragma unroll
      for (int e = 0; e < V; ++e) w[k * V + e] = v[e];
    }
    T fl[I1 - I0], fh[I1 - I0];
#pragma unroll
    for (int i = I0; i < I1; ++i) {
      if (i < L) fl[i - I0] = lo[i];
      if (i < LH) fh[i - I0] = hi[i];
    }
#pragma unroll
    for (int i = I0; i < I1; ++i) {
      if (i < L) vmadd<FMA, kPkFwd>(al, &w[-i * S - A], fl[i - I0]);
      if (i < LH) vmadd<FMA, kPkFwd>(ah, &w[-i * S - A], fh[i - I0]);
    }
  });
}

template <typename T, int L, bool FMA>
__device__ __forceinline__ void fwd_vec(const T* buf, int t0, int S, const T* lo, const T* hi, int taps,
                                        T (&al)[VT<T>::V], T (&ah)[VT<T>::V], int taps_hi = -1) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  if constexpr (L > 0) {
    if (S == 1) { fwd_window<T, L, FMA, 1>(buf, t0, lo, hi, al, ah); return; }
    if constexpr (V == 4) {
      if (S == 2) { fwd_window<T, L, FMA, 2>(buf, t0, lo, hi, al, ah); return; }
    }
#pragma unroll
    for (int i = 0; i < L; ++i) {   // S is a multiple of V: aligned 16-byte reads
      const vec v = *reinterpret_cast<const vec*>(buf + t0 - i * S);
      vmadd<FMA, kPkFwd>(al, v, lo[i]);
      vmadd<FMA, kPkFwd>(ah, v, hi[i]);
    }
  } else {
    // runtime taps; a two-length bank (taps_hi >= 0, != taps): the common taps from one read, then the longer
    // filter's remaining taps alone -- each sum still in ascending tap order
    const int th = taps_hi < 0 ? taps : taps_hi, both = taps < th ? taps : th;
    for (int i = 0; i < both; ++i) {
      const T fl = lo[i], fh = hi[i];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const T xv = buf[t0 + e - i * S];
        al[e] = madd<FMA>(al[e], xv, fl);
        ah[e] = madd<FMA>(ah[e], xv, fh);
      }
    }
    for (int i = both; i < taps; ++i) {
      const T fl = lo[i];
#pragma unroll
      for (int e = 0; e < V; ++e) al[e] = madd<FMA>(al[e], buf[t0 + e - i * S], fl);
    }
    for (int i = both; i < th; ++i) {
      const T fh = hi[i];
#pragma unroll
      for (int e = 0; e < V; ++e) ah[e] = madd<FMA>(ah[e], buf[t0 + e - i * S], fh);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Inverse, one branch: acc_e (+)= f[i] * buf[t0 + e + dir*i*s + off], i ascending
// (MultiLevelMODWTTransform.java:578-588 periodic, :612-639 symmetric orientations).
template <typename T, int L, bool FMA, int S, int DIR>
__device__ __forceinline__ void inv_window(const T* buf, int base, const T* f, T (&acc)[VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  static_for<0, (L + kWinTaps - 1) / kWinTaps>([&](auto c) __attribute__((always_inline)) {
    constexpr int I0 = decltype(c)::value * kWinTaps;
    constexpr int I1 = (I0 + kWinTaps < L) ? I0 + kWinTaps : L;
    // offsets e + DIR*i*S of the chunk's taps, aligned to whole vectors
    constexpr int A = DIR > 0 ? floor_div(I0 * S, V) * V : floor_div(-(I1 - 1) * S, V) * V;
    constexpr int E = DIR > 0 ? (floor_div(V - 1 + (I1 - 1) * S, V) + 1) * V : (floor_div(V - 1 - I0 * S, V) + 1) * V;
    constexpr int NE = E - A;
    T w[NE];
#pragma unroll
    for (int k = 0; k < NE / V; ++k) {
      vec v = *reinterpret_cast<const vec*>(buf + base + A + k * V);
#pragma unroll
      for (int e = 0; e < V; ++e) w[k * V + e] = v[e];
    }
    T fc[I1 - I0];
#pragma unroll
    for (int i = I0; i < I1; ++i) fc[i - I0] = f[i];
#pragma unroll
    for (int i = I0; i < I1; ++i) vmadd<FMA>(acc, &w[DIR * i * S - A], fc[i - I0]);
  });
}

template <typename T, int L, bool FMA>
__device__ __forceinline__ void inv_branch(const T* buf, int t0, int S, int dir, int off, const T* f, int taps,
                                           T (&acc)[VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  if constexpr (L > 0) {
    if ((off & (V - 1)) == 0) {
      const int base = t0 + off;
      if (S == 1) {
        if (dir > 0) inv_window<T, L, FMA, 1, 1>(buf, base, f, acc);
        else inv_window<T, L, FMA, 1, -1>(buf, base, f, acc);
        return;
      }
      if constexpr (V == 4) {
        if (S == 2) {
          if (dir > 0) inv_window<T, L, FMA, 2, 1>(buf, base, f, acc);
          else inv_window<T, L, FMA, 2, -1>(buf, base, f, acc);
          return;
        }
      }
      const int step = dir * S;
#pragma unroll
      for (int i = 0; i < L; ++i) {
        const vec v = *reinterpret_cast<const vec*>(buf + base + i * step);
        vmadd<FMA>(acc, v, f[i]);
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < L; ++i) {
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = madd<FMA>(acc[e], buf[t0 + e + dir * i * S + off], f[i]);
    }
  } else {
    for (int i = 0; i < taps; ++i) {
      const T fi = f[i];
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = madd<FMA>(acc[e], buf[t0 + e + dir * i * S + off], fi);
    }
  }
}

// Pairwise inverse: acc_e += (h[i]*a[idx] + g[i]*d[idx])  (MODWTTransform.java:251-252, :265-266,
// :290-291; MultiLevelMODWTTransform.java:596-597).  idx = t0 + e + dir*i*s.
template <typename T, bool FMA>
__device__ __forceinline__ T pair_term(T h, T a, T g, T d) {
  if constexpr (FMA) return fma_t(h, a, g * d);
  else return h * a + g * d;
}

template <typename T, int L, bool FMA>
__device__ __forceinline__ void inv_pair(const T* A, const T* D, int t0, int S, int dir, const T* h, const T* g,
                                         int taps, T (&acc)[VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  if constexpr (L > 0) {
    if (S % V == 0) {
      const int step = dir * S;
#pragma unroll
      for (int i = 0; i < L; ++i) {
        const vec va = *reinterpret_cast<const vec*>(A + t0 + i * step);
        const vec vd = *reinterpret_cast<const vec*>(D + t0 + i * step);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = acc[e] + pair_term<T, FMA>(h[i], va[e], g[i], vd[e]);
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // <= 8 reads in flight (VGPR budget)
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < L; ++i) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int idx = t0 + e + dir * i * S;
        acc[e] = acc[e] + pair_term<T, FMA>(h[i], A[idx], g[i], D[idx]);
      }
      if ((i & 1) == 1) __builtin_amdgcn_sched_barrier(0);  // bounded reads in flight (VGPR budget)
    }
  } else {
    for (int i = 0; i < taps; ++i) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int idx = t0 + e + dir * i * S;
        acc[e] = acc[e] + pair_term<T, FMA>(h[i], A[idx], g[i], D[idx]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Global <-> register <-> LDS row transfers.  A row is held as NV 16-byte vectors per lane, lane
// `tid` owning vectors w = tid + k*NT (coalesced dwordx4 loads / stores, conflict-free b128 LDS).
//
// Scalar-instruction budget: the scalar unit is shared by the CU's four SIMDs, and per-vector
// runtime checks (bounds, modes, spacing, direction) cost several SALU + a branch each.  So the
// fused kernels make every such decision once per level (row functions below, templated on the
// spacing class and direction), and only the last of a thread's NV vectors carries a bounds check:
// the host sizes the workgroup so that slabs 0..NV-2 are full ((NV-1)*NT <= nvec, vw_plan.cpp fused_plan).
// FULL: every slab is full (threads * NV == nvec, a host contract): no bounds check at all.
template <int L, int NV, bool FULL = false, typename F>
__device__ __forceinline__ void for_vecs(int nvec, F&& fn) {
  const int NT = blockDim.x;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    int w = threadIdx.x + k * NT;
    // Launder w: the addresses derived from it are loop-invariant across the level loop, and
    // hoisting all of them (every vector x every buffer x every spacing path) out of it exhausts
    // the 128-VGPR budget and spills.  Recomputing them per level costs a few VALU.
    asm volatile("" : "+v"(w));
    if (FULL || (L > 0 && k < NV - 1) || w < nvec) fn(k, w);
    // ... and keep the scheduler from issuing the LDS reads of every vector at once (NV x L
    // b128 reads in flight = all the VGPRs); 4 waves per SIMD hide the per-vector read latency.
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Cache policy of the streaming row stores / loads (buffer-instruction aux field: 1 = sc0,
// 2 = nt, 16 = sc1).  VW_STORE_AUX < 0 selects the compiler's nontemporal store.
#ifndef VW_STORE_AUX
#define VW_STORE_AUX -1
#endif
#ifndef VW_LOAD_AUX
#define VW_LOAD_AUX -1
#endif
// Forward coefficient rows (read next by an inverse): sc1.  Same box, alternating, rotated buffer
// sets (profiles/r04/ab_store_policy_*.log): db4 4096 x 4096 42.8-44.0K (nt) -> 45.1-46.0K Msamples/s,
// 512 rows 41.0-41.6K -> 42.9-44.1K; write-back (aux 0) 45.1-45.6K / 40.6-41.1K; sym8 / db8 / coif5
// unchanged (their forwards store through k_forward_blk's write-back path or the tiled kernels).
#ifndef VW_FWD_STORE_AUX
#define VW_FWD_STORE_AUX 16
#endif
#ifndef VW_BLK_NT_M
#define VW_BLK_NT_M 8  // k_forward_blk: vector strides m below this store write-back (see there)
#endif
#ifndef VW_INV_STORE_AUX
#define VW_INV_STORE_AUX VW_STORE_AUX  // inverse output rows
#endif
typedef int vw_i4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, 0x7fffffff, 0x00020000);
}

// base: a workgroup-uniform row pointer; i: the lane's 16-byte vector index within the row.
template <int AUX, typename V16, typename T>
__device__ __forceinline__ void stream_store(T* base, int i, V16 v) {
  if constexpr (AUX < 0) {
    __builtin_nontemporal_store(v, reinterpret_cast<V16*>(base) + i);
  } else {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(vw_i4, v), row_rsrc(base), i * 16, 0, AUX);
  }
}

template <typename V16, typename T>
__device__ __forceinline__ V16 stream_load(const T* base, int i) {
  if constexpr (VW_LOAD_AUX < 0) {
    return __builtin_nontemporal_load(reinterpret_cast<const V16*>(base) + i);
  } else {
    return __builtin_bit_cast(V16, __builtin_amdgcn_raw_buffer_load_b128(row_rsrc(base), i * 16, 0, VW_LOAD_AUX));
  }
}

// FULL: aligned rows of whole vectors (host contract): no ragged-row test, no scalar fallback.
template <int AUX = VW_STORE_AUX, bool FULL = false, typename T>
__device__ __forceinline__ void store_vec(T* __restrict__ dst, int t0, int N, bool vec_ok, const T (&v)[VT<T>::V]) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  if (FULL || (vec_ok && t0 + V <= N)) {
    vec o;
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = v[e];
    stream_store<AUX, vec>(dst, t0 / V, o);
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (t0 + e < N) dst[t0 + e] = v[e];
  }
}

template <typename T>
__device__ __forceinline__ void check_out(int validate, unsigned long long* bad, unsigned long long flat0, int t0,
                                          int N, const T (&v)[VT<T>::V]) {
  if (!validate) return;
  constexpr int V = VT<T>::V;
#pragma unroll
  for (int e = 0; e < V; ++e)
    if (t0 + e < N && !finite_t(v[e])) atomicMin(bad, (1ull << 62) | (flat0 + (unsigned long long)(t0 + e)));
}

// MutableMultiLevelMODWTResult.applyThreshold (:97-114): soft = signum(c)*(|c|-T) above T, hard
// keeps c when |c| > T.
template <typename T>
__device__ __forceinline__ T threshold_t(T c, T thr, int soft) {
  const T av = c < T(0) ? -c : c;
  if (soft) {
    // Math.signum(c) * (|c| - T): c != 0 here, and a product with +-1 is a sign flip, i.e. copysign
    // (c == 0 passes only for a negative threshold: signum(+-0) * x = +-0 * x)
    if (av > thr) return c == T(0) ? c * (av - thr) : __builtin_copysign(av - thr, c);
    return T(0);
  }
  return av <= thr ? T(0) : c;
}

// Issue the loads of one row into registers.  Loads only: the values are first touched where they
// are written to LDS (the zero / threshold selection is applied there), so a prefetch is never
// waited for early.  The vector loads are unconditional (lanes past the row re-read its last vector;
// those registers are never used): an exec-masked load in its own basic block makes the waitcnt
// pass lose count and wait vmcnt(0) at the first use, i.e. for every load in flight.  The unrolled
// kernels (L > 0) only run on 16-byte-aligned rows; the scalar form is the runtime-L kernel's.
template <typename T, int NV, bool FULL = false>
__device__ __forceinline__ void load_row_regs(T (&r)[NV][VT<T>::V], const T* __restrict__ src, int N, int nvec,
                                              bool vec_ok, bool zero) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  const int NT = blockDim.x;
  if (zero) return;  // r stays undefined; the writer substitutes zeros
  if (vec_ok) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      int w = (int)threadIdx.x + k * NT;
      asm volatile("" : "+v"(w));  // not hoisted out of the level loop (see for_vecs)
      if constexpr (!FULL) w = min(w, nvec - 1);
      const vec v = stream_load<vec>(src, w);
#pragma unroll
      for (int e = 0; e < V; ++e) r[k][e] = v[e];
    }
  } else {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int w = threadIdx.x + k * NT;
      if (w < nvec) {
        const int t0 = w * V;
#pragma unroll
        for (int e = 0; e < V; ++e) r[k][e] = (t0 + e < N) ? src[t0 + e] : T(0);
      }
    }
  }
}

// ---- Halo by owner writes ---------------------------------------------------------------------
// Whoever writes element t of a level input into LDS also writes the halo positions the
// reference's index map sends to t, so the halo costs no extra pass and no extra barrier.  With
// hl <= N and hr <= N an element has at most one image per side, an affine function of t:
//   periodic  (i mod N):             t - N (left), t + N (right)
//   symmetric (MathUtils mirror):    -t - 1 (left), 2N - 1 - t (right)
//   fftpad    (i + nextPow2(N) < N):  t - npow2 (left); right halo is zero
// (LevelDesc il_*/ir_*; an image is written when it falls inside [-hl, 0) / [N, N+hr)).  Only
// vectors w < vs (in the thread's first slab) or w >= ve (in its last slab) have images.
// Positions with no source (zero padding, fftpad gaps, streaming history) are written by
// halo_fixed.  When these conditions do not hold the host clears LevelDesc::own and the kernels
// fill the halo from LDS after a barrier (fill_halo), as the reference's modulo does for any index.
template <typename T, bool FULL = false>
__device__ __forceinline__ void halo_images(T* buf, int w, const typename VT<T>::v& o, int N, const LevelDesc& lv) {
  constexpr int V = VT<T>::V;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const int t = w * V + e;
    if (FULL || t < N) {
      const int l = lv.il_a * t + lv.il_b;
      const int r = lv.ir_a * t + lv.ir_b;
      if (l < 0 && l >= -lv.hl) buf[l] = o[e];
      if (r >= N && r < N + lv.hr) buf[r] = o[e];
    }
  }
}

template <typename T>
__device__ __forceinline__ void halo_fixed(T* buf, int N, const LevelDesc& lv, int npow2, const T* hist_b) {
  if (lv.mode == kHaloPeriodic || lv.mode == kHaloSymmetric) return;
  const int total = lv.hl + lv.hr;
  for (int q = threadIdx.x; q < total; q += blockDim.x) {
    const int idx = q < lv.hl ? q - lv.hl : N + (q - lv.hl);
    if (lv.mode == kHaloFftPad && idx < 0 && idx + npow2 < N) continue;  // an element's image
    T v = T(0);
    if (lv.mode == kHaloHistory && idx < 0 && idx >= -lv.hist_len) v = hist_b[lv.hist_len + idx];
    buf[idx] = v;
  }
}

// Write a register-held row into the LDS level buffer `buf` with its halo for level `lv`.
// MODE 0: values as is; 1: zeros (masked-out level, registers never loaded); 2: thresholded.
template <typename T, int L, int NV, int MODE, bool FULL = false>
__device__ __forceinline__ void regs_to_level_m(T* buf, const T (&r)[NV][VT<T>::V], int nvec, int N,
                                                const LevelDesc& lv, T thr_b, int soft) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  const bool own = lv.own != 0;
  for_vecs<L, NV, FULL>(nvec, [&](int k, int w) {
    vec o;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if constexpr (MODE == 1) {
        T z = T(0);
        asm volatile("" : "+v"(z));  // materialised here, not a loop-invariant vector held in VGPRs
        o[e] = z;
      }
      else if constexpr (MODE == 2) o[e] = threshold_t(r[k][e], thr_b, soft);
      else o[e] = r[k][e];
    }
    if (L > 0 || w * V + V <= N) {
      *reinterpret_cast<vec*>(buf + w * V) = o;
    } else {  // ragged tail: positions >= N belong to the right halo (written by their owners)
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (w * V + e < N) buf[w * V + e] = o[e];
    }
    if (own && ((k == 0 && w < lv.vs) || (k == NV - 1 && w >= lv.ve))) halo_images<T, FULL>(buf, w, o, N, lv);
  });
}

// If the level cannot use owner writes this ends with a barrier and the generic halo fill; either
// way the caller's next lds_barrier() publishes data + halo.
template <typename T, int L, int NV, bool FULL = false>
__device__ __forceinline__ void regs_to_level(T* buf, const T (&r)[NV][VT<T>::V], int nvec, int N, const LevelDesc& lv,
                                              int npow2, const T* hist_b, bool zero = false, const T* thr = nullptr,
                                              T thr_b = T(0), int soft = 0) {
  if (zero) regs_to_level_m<T, L, NV, 1, FULL>(buf, r, nvec, N, lv, thr_b, soft);
  else if (thr) regs_to_level_m<T, L, NV, 2, FULL>(buf, r, nvec, N, lv, thr_b, soft);
  else regs_to_level_m<T, L, NV, 0, FULL>(buf, r, nvec, N, lv, thr_b, soft);
  if (lv.own) {
    halo_fixed(buf, N, lv, npow2, hist_b);
  } else {
    lds_barrier();
    fill_halo(buf, N, lv.hl, lv.hr, lv.mode, npow2, hist_b, lv.hist_len);
  }
}

// Counted waits: vmcnt(N) leaves the wave's N youngest vector-memory operations in flight (k_forward_persist,
// k_roundtrip and the deep-level kernels count theirs).
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 0xF) | ((N >> 4) << 14) | (0x7 << 4) | (0xF << 8));
}

// vmcnt(n) for a wave-uniform runtime n (0..63; larger waits for 63, i.e. for more)
__device__ __forceinline__ void wait_vmcnt_rt(int n) {
  // the count is wave-uniform; without this the switch compiles to an exec-masked compare tree on a VGPR
  switch (__builtin_amdgcn_readfirstlane(n)) {
    case 0: wait_vmcnt<0>(); break;
    case 1: wait_vmcnt<1>(); break;
    case 2: wait_vmcnt<2>(); break;
    case 3: wait_vmcnt<3>(); break;
    case 4: wait_vmcnt<4>(); break;
    case 5: wait_vmcnt<5>(); break;
    case 6: wait_vmcnt<6>(); break;
    case 7: wait_vmcnt<7>(); break;
    case 8: wait_vmcnt<8>(); break;
    case 9: wait_vmcnt<9>(); break;
    case 10: wait_vmcnt<10>(); break;
    case 11: wait_vmcnt<11>(); break;
    case 12: wait_vmcnt<12>(); break;
    case 13: wait_vmcnt<13>(); break;
    case 14: wait_vmcnt<14>(); break;
    case 15: wait_vmcnt<15>(); break;
    case 16: wait_vmcnt<16>(); break;
    case 17: wait_vmcnt<17>(); break;
    case 18: wait_vmcnt<18>(); break;
    case 19: wait_vmcnt<19>(); break;
    case 20: wait_vmcnt<20>(); break;
    case 21: wait_vmcnt<21>(); break;
    case 22: wait_vmcnt<22>(); break;
    case 23: wait_vmcnt<23>(); break;
    case 24: wait_vmcnt<24>(); break;
    case 25: wait_vmcnt<25>(); break;
    case 26: wait_vmcnt<26>(); break;
    case 27: wait_vmcnt<27>(); break;
    case 28: wait_vmcnt<28>(); break;
    case 29: wait_vmcnt<29>(); break;
    case 30: wait_vmcnt<30>(); break;
    case 31: wait_vmcnt<31>(); break;
    case 32: wait_vmcnt<32>(); break;
    case 33: wait_vmcnt<33>(); break;
    case 34: wait_vmcnt<34>(); break;
    case 35: wait_vmcnt<35>(); break;
    case 36: wait_vmcnt<36>(); break;
    case 37: wait_vmcnt<37>(); break;
    case 38: wait_vmcnt<38>(); break;
    case 39: wait_vmcnt<39>(); break;
    case 40: wait_vmcnt<40>(); break;
    case 41: wait_vmcnt<41>(); break;
    case 42: wait_vmcnt<42>(); break;
    case 43: wait_vmcnt<43>(); break;
    case 44: wait_vmcnt<44>(); break;
    case 45: wait_vmcnt<45>(); break;
    case 46: wait_vmcnt<46>(); break;
    case 47: wait_vmcnt<47>(); break;
    case 48: wait_vmcnt<48>(); break;
    case 49: wait_vmcnt<49>(); break;
    case 50: wait_vmcnt<50>(); break;
    case 51: wait_vmcnt<51>(); break;
    case 52: wait_vmcnt<52>(); break;
    case 53: wait_vmcnt<53>(); break;
    case 54: wait_vmcnt<54>(); break;
    case 55: wait_vmcnt<55>(); break;
    case 56: wait_vmcnt<56>(); break;
    case 57: wait_vmcnt<57>(); break;
    case 58: wait_vmcnt<58>(); break;
    case 59: wait_vmcnt<59>(); break;
    case 60: wait_vmcnt<60>(); break;
    case 61: wait_vmcnt<61>(); break;
    case 62: wait_vmcnt<62>(); break;
    case 63: wait_vmcnt<63>(); break;
    default: wait_vmcnt<63>(); break;
  }
}

template <typename T, int NV>
__device__ __forceinline__ void zero_regs(T (&r)[NV][VT<T>::V]) {
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int e = 0; e < VT<T>::V; ++e) r[k][e] = T(0);
}

// Launch bounds of the fused kernels.  NV = 4: at most 512 threads and W waves per SIMD -- W = 8
// (64 VGPRs: four 512-thread workgroups per CU, LDS permitting) for the forward, W = 6 (80 VGPRs,
// three workgroups) for the inverses, whose prefetched detail row occupies 16 more VGPRs -- so
// several workgroups share a CU and hide each other's barriers and row loads.  The one inverse that
// also exists at W = 8 is k_inverse_seq's PLAIN form (fp64, L <= 8; inverse_seq_plain): it fits 64 VGPRs
// without scratch, and VW_INV_WAVES picks between its two instantiations.  NV = 8 (long
// signals): up to 1024 threads, 128 VGPRs.
// Longer filters need wider register windows (the s = 1 window holds L + V - 1 values): L <= 8 gets
// W waves, longer filters 4 (128 VGPRs; with 512-thread workgroups 5 waves would not add one).
// NV = 2 (small batches: one 1024-thread workgroup per signal, two per CU = 8 waves per SIMD, 64 VGPRs):
// twice the waves per signal where the batch leaves the CUs short of signals.
#ifndef VW_LONG_WAVES
#define VW_LONG_WAVES 4  // waves per SIMD the fused kernels of long filters (L > 8) are compiled for
#endif
#define VW_FUSED_W(L, W) ((L) <= 8 ? (W) : VW_LONG_WAVES)
#define VW_FUSED_BOUNDS(NV, W)                                                        \
  __attribute__((amdgpu_flat_work_group_size(1, ((NV) <= 4 && (NV) != 2) ? 512 : 1024), \
                 amdgpu_waves_per_eu((NV) == 2 ? 8 : (NV) <= 4 ? (W) : 4)))

// ---------------------------------------------------------------------------------------------
// Non-finite probe (VW_FLAG_REF_NONFINITE, vw_ref.hip): z = v * 0 + z stays +-0 while every v is finite
// and becomes NaN for good at the first NaN / +-Inf -- one FMA per value, no compare or mask in the loop.
template <typename T>
__device__ __forceinline__ T nf_step(T v, T z) {
  if constexpr (sizeof(T) == 8) return __builtin_fma(v, T(0), z);
  else return __builtin_fmaf(v, T(0), z);
}
template <typename T, int V>
__device__ __forceinline__ void nf_probe(T& z, const T (&v)[V]) {
#pragma unroll
  for (int e = 0; e < V; ++e) z = nf_step<T>(v[e], z);
}
// a row in registers (load_row_regs layout): only the vectors the thread holds (for_vecs)
template <typename T, int L, int NV, int V, bool FULL = false>
__device__ __forceinline__ void nf_probe_rows(T& z, const T (&v)[NV][V], int nvec) {
  for_vecs<L, NV, FULL>(nvec, [&](int k, int) { nf_probe<T, V>(z, v[k]); });
}
// row b flagged when any lane of any wave saw one (a plain vector store: every writer stores the same 1)
template <typename T>
__device__ __forceinline__ void nf_flag_row(int* flag, long long b, T z) {
  if (__any(z != z) && (threadIdx.x & 63) == 0) flag[b] = 1;
}

}  // namespace vw
