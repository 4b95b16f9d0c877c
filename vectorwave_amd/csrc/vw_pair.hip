// vw_pair.hip -- k_roundtrip: the forward and the inverse of the same rows in one persistent launch (fp64, L <= 8,
// PERIODIC; vw_plan.cpp pair_fusable names the pairs of calls it replaces).
//
// A workgroup walks rows b = blockIdx.x, + gridDim.x, ... as k_forward_persist does.  Per row:
//   forward half  k_forward_persist<T, L, FMA, 4, FULL = true>'s loop body: fwd_level / regs_to_level, the LDS-DMA
//                 of the next row into the free buffer during level J, d_1 .. d_J and a_J stored to the caller's
//                 planes -- every output of the forward call is written;
//   inverse half  inverse_seq_plain's schedule, phase for phase (plain_to_level, plain_row: taps ascending, the
//                 approximation branch before the detail branch), in the level buffer that is dead after level J's
//                 reads while the other buffer receives the next row.
// The inverse half's operands: a_J is the forward's areg and d_J the detail vectors fwd_level keeps at level J --
// neither is loaded.  KEEP (0, 1 or 2) more detail planes stay in registers as well: ahead of each level the forward
// half shifts dk[1] = dk[0], dk[0] = dlast (compile-time indices: nothing becomes addressable), so that after level
// J dk[q] holds d_{J-1-q}; every plane is still stored as before.  The other planes, d_{J-1-KEEP} .. d_1, come back
// through plain_load_row, one level ahead, with loads that bypass L1.  KEEP = 0 is the kernel as it was; the host
// picks KEEP (pair_keep_variant, vw_plan.cpp) so that a kept plane never costs a resident workgroup.
// OWNERSHIP: both halves give lane tid the vectors tid + k * blockDim.x, k = 0 .. 3 -- for_vecs computes
// w = threadIdx.x + k * blockDim.x, plain_vecs / plain_load_row the byte offset threadIdx.x * 16 + k * slab with
// slab = blockDim.x * 16 -- so each lane reads back exactly the 16-byte vectors it stored itself, and a row never
// leaves its workgroup: no fence, flag or cross-workgroup hand-off.  What orders a lane's reload behind its own
// store is a counted vmcnt wait (vmcnt retires a wave's vector-memory operations in issue order).  The first
// reload is of d_{J-1-KEEP}, issued at level j = J - KEEP of the inverse half (J >= KEEP + 2).  After that plane's
// stores the wave has issued the KEEP * NV stores of the kept planes d_{J-KEEP} .. d_{J-1}, then the next row's DMA
// (NV instructions, when there is a next row), then level J's 2 * NV stores, and nothing since: the inverse half
// issues no vector-memory operation before its first reload.  vmcnt(3 * NV) resp. vmcnt(2 * NV) leaves at most the
// DMA and level J's stores in flight, so it retires the stores of d_1 .. d_{J-1}, the reloaded plane's among them
// (and with them the kept planes', which is more than needed and by then long done).  Every later reload follows
// inverse_seq_plain's vmcnt(0).  When J <= KEEP + 1 nothing is reloaded and no vmcnt(0) happens; the row loop's
// closing vmcnt(3 * NV) then retires the DMA by itself: behind it the wave issued level J's 2 * NV stores and the
// NV stores of y, as at J = 1 without kept planes.
// Per output the operation sequence of both halves is that of the two separate kernels: every array is
// bit-identical to theirs in both accumulation modes.
//
// LDS: the forward's two regions (hlpad + N + V elements each), unchanged.  The forward reads [-hl, N) of a region's
// element 0 = region start + hlpad; the inverse reads [0, N + hr) from the region start, hr <= hlpad (both are
// (L - 1) * 2^(J-1) rounded: pair_fusable checks it) -- the size is the maximum of the two needs, not their sum.
// Registers: 4 waves per SIMD (128 VGPRs) as the forward; the halves are sequential.  A kept plane is 16 VGPRs:
// KEEP = 2 takes 124-125 of the 128 at L = 8, a third plane spills.
#include "vw_launch_k.h"
#include "vw_dev_fwd.h"
#include "vw_dev_inv.h"

#include <algorithm>
#include <mutex>

namespace vw {

// Cache policy of k_roundtrip's coefficient stores (buffer aux: 0 = write-back, 2 = nt, 16 = sc1; see VW_FWD_STORE_AUX).
#ifndef VW_PAIR_STORE_AUX
#define VW_PAIR_STORE_AUX 16
#endif

// p again, through an offset the compiler cannot see through: what is read behind the result is loaded where it is
// used.  The four filters of a round trip are 8 * L SGPRs; hoisted out of the row loop together (they are kernel
// arguments, so every read of them is loop-invariant) they spill.
template <typename P>
__device__ __forceinline__ const P* reread(const P* p) {
  int z = 0;
  asm volatile("" : "+s"(z));
  return p + z;
}

// to = from, vector for vector (the kept planes' shift: compile-time indices only)
template <typename T, int NV>
__device__ __forceinline__ void copy_regs(T (&to)[NV][VT<T>::V], const T (&from)[NV][VT<T>::V]) {
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int e = 0; e < VT<T>::V; ++e) to[k][e] = from[k][e];
}

// KEEP = 0 keeps the name and the parameters it has had (profiles and the resource checks name it); the variants
// with kept planes are k_rtrip_keep.  One body: vw_pair_rows.inc.
template <typename T, int L, bool FMA>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, 512), amdgpu_waves_per_eu(4)))
k_roundtrip(const PairArgs<T> q) {
  constexpr int KEEP = 0;
#include "vw_pair_rows.inc"
}

template <typename T, int L, bool FMA, int KEEP>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, 512), amdgpu_waves_per_eu(4)))
k_rtrip_keep(const PairArgs<T> q) {
  static_assert(KEEP >= 1 && KEEP <= kPairMaxKeep, "KEEP = 0 is k_roundtrip; a third kept plane spills");
#include "vw_pair_rows.inc"
}

// One kernel per (taps, accumulation mode, kept planes); resident workgroups per CU from the occupancy API, as
// run_forward_persist takes its grid: one query per (threads, LDS) shape, the last kShapes shapes kept (several
// contexts, each on a host thread of its own, may prepare and record at once).
struct PairKernel {
  static constexpr int kShapes = 16;
  const void* func = nullptr;
  LdsOnce lds;
  std::mutex mu;
  struct Shape { int threads = -1, lds = -1, per_cu = 0; } shapes[kShapes];
  int next = 0;
  int find(int threads, int lds_bytes) {  // mu held; resident workgroups per CU, 0 = not queried
    for (const Shape& sh : shapes)
      if (sh.threads == threads && sh.lds == lds_bytes) return sh.per_cu;
    return 0;
  }
};

template <int L, bool FMA, int KEEP>
static PairKernel* pair_kernel_of() {
  static PairKernel k;
  if constexpr (KEEP == 0) k.func = reinterpret_cast<const void*>(&k_roundtrip<double, L, FMA>);
  else k.func = reinterpret_cast<const void*>(&k_rtrip_keep<double, L, FMA, KEEP>);
  return &k;
}

template <int L, bool FMA>
static PairKernel* pair_kernel_keep(int keep) {
  static_assert(kPairMaxKeep == 2, "one case per variant");
  return keep == 0 ? pair_kernel_of<L, FMA, 0>() : keep == 1 ? pair_kernel_of<L, FMA, 1>() : pair_kernel_of<L, FMA, 2>();
}

static PairKernel* pair_kernel(int taps, bool fma, int keep) {
  if (keep < 0 || keep > kPairMaxKeep) return nullptr;
  PairKernel* k = nullptr;  // stays null for an unlisted count, or one above kPairMaxTaps
  (void)dispatch_taps<Unlisted::kNotSupported, kPairMaxTaps>(taps, fma, [&](auto l, auto m) {
    k = pair_kernel_keep<l(), m()>(keep);
    return hipSuccess;
  });
  return k;
}

// the dynamic-LDS limit of this device's copy of the kernel covers `lds` (vw_launch_k.h set_lds)
static bool lds_ready(PairKernel* k, int lds) {
  if (lds <= 64 * 1024) return true;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return false;
  return k->lds.limit[dev].load(std::memory_order_acquire) >= lds;
}

// one variant's share of pair_prepare: its LDS limit, and its occupancy for the shape (queried once)
static hipError_t prepare_variant(PairKernel* k, int threads, int lds, int* per_cu) {
  hipError_t e = set_lds(k->func, lds, &k->lds);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> g(k->mu);
  int n = k->find(threads, lds);
  if (!n) {
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k->func, threads, lds)) != hipSuccess) return e;
    if (n < 1) return hipErrorInvalidConfiguration;
    PairKernel::Shape& sh = k->shapes[k->next];
    k->next = (k->next + 1) % PairKernel::kShapes;
    sh.threads = threads; sh.lds = lds; sh.per_cu = n;
  }
  *per_cu = n;
  return hipSuccess;
}

// Every variant is prepared, whichever is asked for: the auto rule (pair_keep_variant) compares their occupancies,
// and a context that forces another variant later finds it ready while capturing.
hipError_t pair_prepare(int taps, bool fma, int threads, int lds, int keep, int* per_cu, int* variant) {
  int n[kPairMaxKeep + 1];
  for (int v = 0; v <= kPairMaxKeep; ++v) {
    PairKernel* k = pair_kernel(taps, fma, v);
    if (!k) return hipErrorNotSupported;
    hipError_t e = prepare_variant(k, threads, lds, &n[v]);
    if (e != hipSuccess) return e;
  }
  const int v = pair_keep_variant(keep, n);
  if (per_cu) *per_cu = n[v];
  if (variant) *variant = v;
  return hipSuccess;
}

bool pair_launch_shape(int taps, bool fma, int threads, int lds, int keep, long long B, int cus, PairLaunch* out) {
  int n[kPairMaxKeep + 1];
  PairKernel* ks[kPairMaxKeep + 1];
  for (int v = 0; v <= kPairMaxKeep; ++v) {
    PairKernel* k = ks[v] = pair_kernel(taps, fma, v);
    if (!k || !lds_ready(k, lds)) return false;
    std::lock_guard<std::mutex> g(k->mu);
    if ((n[v] = k->find(threads, lds)) < 1) return false;
  }
  const int v = pair_keep_variant(keep, n);
  out->func = ks[v]->func;
  out->grid = (unsigned)std::min<long long>(B, (long long)n[v] * cus);
  out->threads = (unsigned)threads;
  out->lds = (unsigned)lds;
  out->keep = v;
  out->per_cu = n[v];
  return true;
}

hipError_t launch_roundtrip(const PairArgs<double>& a, const PairLaunch& l, hipStream_t st) {
  void* params[] = {const_cast<PairArgs<double>*>(&a)};
  return hipLaunchKernel(l.func, dim3(l.grid), dim3(l.threads), params, l.lds, st);
}

}  // namespace vw
