#pragma once
// vw_dev_fwd.h -- the fused forward family: fwd_level, k_forward_fused, the LDS-DMA helpers, k_forward_persist.
// Launched by vw_fwd.hip; vw_pair.hip's k_roundtrip runs the same pieces as its forward half.
#include "vw_dev_rows.h"

#pragma clang fp contract(off)

namespace vw {

// ---------------------------------------------------------------------------------------------
// Fused multi-level forward: MultiLevelMODWTTransform.decompose (:243-251) / BatchSIMDMODWT
// .batchMultiLevelMODWTSoA (:362-377) / VectorWaveSwtAdapter.decomposeSWT (:370-390) /
// BatchStreamingMODWT.processMultiLevel (:130-158) for one signal per workgroup.
//
// Level inputs alternate between two LDS buffers (p.region1 != 0): level j reads X while its
// approximation -- the input of level j+1, halo included -- is written into Y, so each level costs
// ONE workgroup barrier.  With one buffer (long signals), a second barrier guards the overwrite.
// NFP: probe the final approximation (nf: the row's accumulator, see nf_probe)
// AUX: cache policy of the coefficient stores.  dkeep (k_roundtrip): where the level's detail vectors stay in
// registers besides being stored, in areg's layout (nullptr: nowhere).
// INSTRUCTION COUNT: in the FULL form a lane issues exactly one vector-memory store per store_vec below, i.e. NV per
// level and 2 * NV at the level that also writes aout, and nothing else.  The counted vmcnt waits of
// k_forward_persist and k_roundtrip (vw_pair.hip: its first reload, of d_{J-1-KEEP}, behind the lane's own stores -- the
// KEEP * NV stores of the kept planes' levels, then level J's 2 * NV, are all that follows that plane's) depend on it.
template <typename T, int L, bool FMA, int NV, bool VALIDATE, bool NFP = false, bool FULL = false, int LH = L,
          int AUX = VW_FWD_STORE_AUX>
__device__ __forceinline__ void fwd_level(const FwdArgs<T>& p, const T* X, int nvec, const LevelDesc& lv, T* dout,
                                          T* aout, bool vec_ok, unsigned long long flat0, T (&areg)[NV][VT<T>::V],
                                          T* nf = nullptr, T (*dkeep)[VT<T>::V] = nullptr) {
  constexpr int V = VT<T>::V;
  const int N = p.N;
  // (the validating form keeps the run-time-stride body: one level body per kernel is enough there)
  const int ct = VALIDATE ? 0 : p.level_ct;
  fwd_row<T, L, FMA, NV, FULL, LH>(X, nvec, lv.s, p.lo, p.hi, p.taps, ct, [&](int k, int w, const T (&al)[V], const T (&ah)[V]) {
    const int t0 = w * V;
    store_vec<AUX, FULL>(dout, t0, N, vec_ok, ah);
    if (aout) store_vec<AUX, FULL>(aout, t0, N, vec_ok, al);
    if constexpr (VALIDATE) {
      check_out<T>(1, p.bad, flat0, t0, N, ah);
      check_out<T>(1, p.bad, flat0, t0, N, al);
    }
    if constexpr (NFP) {
      if (aout) nf_probe<T, V>(*nf, al);  // a_J suffices (k_forward_persist; vw_ref.hip)
    }
#pragma unroll
    for (int e = 0; e < V; ++e) areg[k][e] = al[e];
    if (dkeep) {
#pragma unroll
      for (int e = 0; e < V; ++e) dkeep[k][e] = ah[e];
    }
  }, p.taps_hi);
}

// HIST: streaming history halos (kHaloHistory) possible.  The history is the only global load inside
// the level loop; without it (HIST = false) no load can be pending there, so the waitcnt pass never
// waits vmcnt(0) -- which on gfx950 would also wait for every detail store still in flight.
// LH: the high-pass tap count of a two-length bank (VW_BI; fwd_window); LH = L is the equal-length kernel.
template <typename T, int L, bool FMA, int NV, bool HIST, int LH = L>
__global__ void VW_FUSED_BOUNDS(NV, VW_FUSED_W((L > LH ? L : LH), 8)) k_forward_fused(const FwdArgs<T> p) {
  constexpr int V = VT<T>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* X = reinterpret_cast<T*>(smem) + p.hlpad;
  T* Y = p.region1 ? reinterpret_cast<T*>(smem) + p.region1 + p.hlpad : X;
  const bool dbl = p.region1 != 0;
  const long long b = p.rev ? p.B - 1 - (long long)blockIdx.x : (long long)blockIdx.x;
  const int N = p.N;
  const int nvec = (N + V - 1) / V;
  const int NT = blockDim.x;
  const int tid = threadIdx.x;
  const bool vec_ok = (L > 0) || p.vec_io != 0;  // unrolled kernels run with aligned rows only
  const unsigned long long flat0 = (unsigned long long)b * (unsigned long long)N;
  auto hist_of = [&](int j) -> const T* {  // level j's streaming history row (or nullptr)
    if constexpr (!HIST) return nullptr;
    const LevelDesc& d = p.lv[j - 1];
    return d.mode == kHaloHistory ? p.hist[j - 1] + b * d.hist_len : nullptr;
  };

  T areg[NV][V];
  load_row_regs<T, NV>(areg, p.x + b * p.ldx, N, nvec, vec_ok, false);
  wait_vmem();
  if (p.validate) {
    for_vecs<L, NV>(nvec, [&](int k, int w) {
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (w * V + e < N && !finite_t(areg[k][e])) atomicMin(p.bad, flat0 + (unsigned long long)(w * V + e));
    });
  }
  regs_to_level<T, L, NV>(X, areg, nvec, N, p.lv[0], p.npow2, hist_of(1));

  for (int j = 1; j <= p.J; ++j) {
    const LevelDesc lv = p.lv[j - 1];
    lds_barrier();  // X = level input + halo; every read of Y (previous level) done
    T* dout = p.details + ((size_t)(j - 1) * (size_t)p.B + (size_t)b) * (size_t)N;
    T* aout = (j == p.J) ? p.approx + b * (size_t)N : nullptr;
    if (p.validate) fwd_level<T, L, FMA, NV, true, false, false, LH>(p, X, nvec, lv, dout, aout, vec_ok, flat0, areg);
    else fwd_level<T, L, FMA, NV, false, false, false, LH>(p, X, nvec, lv, dout, aout, vec_ok, flat0, areg);
    // Streaming: new left history = last hist_len samples of this level's input
    // (BatchStreamingMODWT.updateHistoryFromSoA :337-352).
    if (HIST && p.hist_update && lv.hist_len > 0) {
      T* hnew = p.hist[j - 1] + b * lv.hist_len;
      for (int q = tid; q < lv.hist_len; q += NT) hnew[q] = X[q + N - lv.hist_len];
    }
    if (j < p.J) {
      if (!dbl) lds_barrier();  // one buffer: every read of this level's input done first
      regs_to_level<T, L, NV>(Y, areg, nvec, N, p.lv[j], p.npow2, hist_of(j + 1));
      T* t = X; X = Y; Y = t;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Persistent fused forward: the same cascade as k_forward_fused, but each workgroup walks the
// signals b = blockIdx.x, + gridDim.x, ... and copies the NEXT signal's row into LDS while the
// current one computes its last level.  With two level buffers, level J reads X and writes no next
// level, so the other buffer is free from its first barrier on: the row goes there by LDS-DMA
// (global_load_lds_dwordx4, no VGPRs), overlapping the read of x with level J's arithmetic and
// detail stores instead of starting every signal with an exposed load (one workgroup per signal
// waits for its row before any store can be issued; at 2 workgroups per CU both often wait at once).
//
// The DMA is issued from inline asm so the compiler does not pessimistically wait for it before the
// LDS reads of level J (it cannot prove the buffers disjoint).  Completion is waited for explicitly:
// vmcnt counts a wave's vector-memory operations in issue order, and exactly 2*NV stores (detail +
// approximation rows) follow the DMA, so vmcnt(2*NV) retires the DMA and leaves those stores in
// flight.  Host contract (vw_plan.cpp plan_forward_fused): two buffers, every slab full (threads*NV == N/V), whole
// waves, N/V a multiple of 64 (one wave instruction = 64 x 16 B), no validation, no history.
// One wave instruction of LDS-DMA: 64 lanes x 16 bytes from per-lane global addresses into 1 KiB of
// LDS at the wave-uniform byte address `lds` (global_load_lds_dwordx4; no VGPR is written).  nt: the
// non-temporal cache policy (a row read once by this launch need not be kept in L2 / Infinity Cache).
// Issued from inline asm so the compiler's waitcnt pass does not wait for it before unrelated LDS
// reads; the caller retires it with an explicit vmcnt wait.
__device__ __forceinline__ void lds_dma16(unsigned lds, const void* g, bool nt) {
  unsigned keep;
  if (nt) {
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off nt\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(g), "s"(__builtin_amdgcn_readfirstlane(lds))
        : "memory");
  } else {
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(g), "s"(__builtin_amdgcn_readfirstlane(lds))
        : "memory");
  }
}

// INSTRUCTION COUNT: under the full-slab contract (threads * NV == nvec, whole waves) a wave issues exactly NV of
// these.  k_forward_persist's vmcnt(2 * NV) and k_roundtrip's vmcnt(3 * NV) / vmcnt(2 * NV) (vw_pair.hip: ahead of its
// first reload, and closing the row where nothing is reloaded, J <= KEEP + 1) count on it.
template <typename T>
__device__ __forceinline__ void dma_row(T* buf, const T* __restrict__ src, int nvec, bool nt) {
  constexpr int V = VT<T>::V;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  for (int c = wv; c * 64 < nvec; c += nw)
    lds_dma16((unsigned)(uintptr_t)(buf + c * 64 * V), src + (size_t)(c * 64 + lane) * V, nt);
}

// FULL: the launch contract above (aligned rows, every slab full) used at compile time -- no per-vector
// w < nvec mask, no ragged-row test or scalar fallback around the stores (VW_LEVEL_CT; FULL = false keeps
// the checks of the shared row functions, which can never fire here).
template <typename T, int L, bool FMA, int NV, bool FULL>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, NV <= 4 ? 512 : 1024), amdgpu_waves_per_eu(4)))
k_forward_persist(const FwdArgs<T> p) {
  constexpr int V = VT<T>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* const B0 = reinterpret_cast<T*>(smem) + p.hlpad;  // (no pointer array: it would lose the LDS address space)
  T* const B1 = reinterpret_cast<T*>(smem) + p.region1 + p.hlpad;
  const int N = p.N;
  const int nvec = N / V;
  const long long G = gridDim.x;
  long long b = blockIdx.x;
  if (b >= p.B) return;
  int cur = 0;
  T nf = T(0);
  dma_row<T>(B0, p.x + b * p.ldx, nvec, p.dma_nt != 0);
  wait_vmem();
  for (;;) {
    T* X = cur ? B1 : B0;
    T* Y = cur ? B0 : B1;
    lds_barrier();  // the row is in X (every wave's share); every read of the previous signal done
    const LevelDesc lv0 = p.lv[0];
    fill_halo(X, N, lv0.hl, lv0.hr, lv0.mode, p.npow2, (const T*)nullptr, 0);
    const long long bn = b + G;
    T areg[NV][V];
    for (int j = 1; j <= p.J; ++j) {
      const LevelDesc lv = p.lv[j - 1];
      lds_barrier();  // X = level input + halo; every read of Y (previous level) done
      if (j == p.J && bn < p.B) {
        dma_row<T>(Y, p.x + bn * p.ldx, nvec, p.dma_nt != 0);  // next signal -> free buffer
      }
      T* dout = p.details + ((size_t)(j - 1) * (size_t)p.B + (size_t)b) * (size_t)N;
      T* aout = (j == p.J) ? p.approx + b * (size_t)N : nullptr;
      if (p.nf_flag) fwd_level<T, L, FMA, NV, false, true, FULL>(p, X, nvec, lv, dout, aout, true, 0ull, areg, &nf);
      else fwd_level<T, L, FMA, NV, false, false, FULL>(p, X, nvec, lv, dout, aout, true, 0ull, areg);
      if (j < p.J) {
        regs_to_level<T, L, NV, FULL>(Y, areg, nvec, N, p.lv[j], p.npow2, (const T*)nullptr);
        T* t = X; X = Y; Y = t;
      }
    }
    // VW_FLAG_REF_NONFINITE: probing a_J flags every row vw_ref.hip must recompute (see there)
    if (p.nf_flag) {
      nf_flag_row<T>(p.nf_flag, b, nf);
      nf = T(0);
    }
    if (bn >= p.B) break;
    wait_vmcnt<2 * NV>();  // this wave's DMA share landed; level J's stores stay in flight
    cur = (cur + p.J) & 1;  // the buffer that was free during level J
    b = bn;
  }
}
}  // namespace vw
