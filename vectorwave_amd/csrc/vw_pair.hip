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
// neither is loaded.  d_{J-1} .. d_1 come back through plain_load_row, one level ahead, with loads that bypass L1.
// OWNERSHIP: both halves give lane tid the vectors tid + k * blockDim.x, k = 0 .. 3 -- for_vecs computes
// w = threadIdx.x + k * blockDim.x, plain_vecs / plain_load_row the byte offset threadIdx.x * 16 + k * slab with
// slab = blockDim.x * 16 -- so each lane reads back exactly the 16-byte vectors it stored itself, and a row never
// leaves its workgroup: no fence, flag or cross-workgroup hand-off.  What orders a lane's reload behind its own
// store is a counted vmcnt wait (vmcnt retires a wave's vector-memory operations in issue order): before the first
// reload, of d_{J-1}, the wave has issued after d_{J-1}'s stores only the next row's DMA (NV instructions, when
// there is a next row) and level J's 2 * NV stores, so vmcnt(3 * NV) resp. vmcnt(2 * NV) covers the stores of
// d_1 .. d_{J-1}.  Every later reload follows inverse_seq_plain's vmcnt(0).
// Per output the operation sequence of both halves is that of the two separate kernels: every array is
// bit-identical to theirs in both accumulation modes.
//
// LDS: the forward's two regions (hlpad + N + V elements each), unchanged.  The forward reads [-hl, N) of a region's
// element 0 = region start + hlpad; the inverse reads [0, N + hr) from the region start, hr <= hlpad (both are
// (L - 1) * 2^(J-1) rounded: pair_fusable checks it) -- the size is the maximum of the two needs, not their sum.
// Registers: 4 waves per SIMD (128 VGPRs) as the forward; the halves are sequential.
#include "vw_device.h"

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

template <typename T, int L, bool FMA>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, 512), amdgpu_waves_per_eu(4)))
k_roundtrip(const PairArgs<T> q) {
  constexpr int V = VT<T>::V;
  constexpr int NV = 4;
  const FwdArgs<T>& p = q.f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int N = p.N;
  const int nvec = N / V;
  const long long G = gridDim.x;
  const size_t plane = (size_t)p.B * (size_t)(unsigned)p.N;
  const unsigned slab = blockDim.x * 16u;  // bytes between a lane's vectors
  long long b = blockIdx.x;
  if (b >= p.B) return;
  int cur = 0;
  dma_row<T>(reinterpret_cast<T*>(smem) + p.hlpad, p.x + b * p.ldx, nvec, p.dma_nt != 0);
  wait_vmem();
  for (;;) {
    const FwdArgs<T>& p0 = *reread(&q.f);  // the row's share of the arguments, read here (as every level's below)
    T* X = reinterpret_cast<T*>(smem) + (cur ? p0.region1 : 0) + p0.hlpad;
    T* Y = reinterpret_cast<T*>(smem) + (cur ? 0 : p0.region1) + p0.hlpad;
    lds_barrier();  // the row is in X (every wave's share); every read of the previous row done
    fill_halo(X, p0.N, p0.lv[0].hl, p0.lv[0].hr, p0.lv[0].mode, p0.npow2, (const T*)nullptr, 0);
    const long long bn = b + G;
    const size_t row = (size_t)b * (size_t)(unsigned)N;
    const int J = p0.J;
    T acc[NV][V];   // forward: the running approximation; inverse: a_J, then the sums
    T dlast[NV][V];  // d_J, kept from level J of the forward.  Every level writes it and the last one stays: handing
                     // fwd_level `j == J ? dlast : nullptr` makes the array's address a run-time value, and the
                     // compiler then keeps it in scratch (80 bytes per lane) instead of 16 VGPRs
    T dreg[NV][V];   // the prefetched d_{j-1}: never written but by its loads, so that no wait the compiler derives
                     // for those registers lands in the forward half or ahead of d_J's use, behind the stores in flight
    // ---- forward half (k_forward_persist) ----
    for (int j = 1; j <= J; ++j) {
      const FwdArgs<T>& pj = *reread(&q.f);  // this level's share of the arguments, read here
      const LevelDesc lv = pj.lv[j - 1];
      lds_barrier();  // X = level input + halo; every read of Y (previous level) done
      if (j == pj.J && bn < pj.B) dma_row<T>(Y, pj.x + bn * pj.ldx, nvec, pj.dma_nt != 0);  // next row -> free buffer
      T* dout = pj.details + (size_t)(j - 1) * plane + row;
      T* aout = (j == pj.J) ? pj.approx + row : nullptr;
      fwd_level<T, L, FMA, NV, false, false, true, L, VW_PAIR_STORE_AUX>(p, X, nvec, lv, dout, aout, true, 0ull, acc,
                                                                         nullptr, dlast);
      if (j < pj.J) {
        regs_to_level<T, L, NV, true>(Y, acc, nvec, pj.N, pj.lv[j], pj.npow2, (const T*)nullptr);
        T* t = X; X = Y; Y = t;
      }
    }
    // ---- inverse half (inverse_seq_plain); X: level J's input, Y: receiving the next row ----
    const PairArgs<T>& qi = *reread(&q);
    T* const R = X - qi.f.hlpad;
    lds_barrier();  // every level-J read of X done
    plain_to_level<T, NV>(R, acc, slab, qi.f.N, qi.hr[qi.f.J - 1], qi.own[qi.f.J - 1]);
    for (int j = J; j >= 1; --j) {
      const PairArgs<T>& qj = *reread(&q);
      const int s = qj.f.lv[j - 1].s;
      lds_barrier();  // R = a_j + halo
      zero_regs<T, NV>(acc);
      plain_row<T, L, FMA, NV, 4>(R, slab, s, qj.ilo, acc);
      lds_barrier();  // every approximation-branch read done
      if (j < qj.f.J) {
        wait_vmem();  // the d_j prefetch
        plain_to_level<T, NV>(R, dreg, slab, qj.f.N, qj.hr[j - 1], qj.own[j - 1]);
      } else {  // d_J never left the registers
        plain_to_level<T, NV>(R, dlast, slab, qj.f.N, qj.hr[j - 1], qj.own[j - 1]);
      }
      if (j > 1) {  // the d_{j-1} prefetch, in flight across the detail branch
        if (j == qj.f.J) {  // behind this lane's own stores of d_1 .. d_{J-1} (see OWNERSHIP above)
          if (bn < qj.f.B) wait_vmcnt<3 * NV>();
          else wait_vmcnt<2 * NV>();
        }
        plain_load_row<T, NV>(dreg, qj.f.details + (size_t)(j - 2) * plane + row, slab);
      }
      lds_barrier();  // R = d_j + halo
      plain_row<T, L, FMA, NV, 4>(R, slab, s, reread(q.ihi), acc);
      if (j > 1) {
        lds_barrier();  // every detail-branch read done
        plain_to_level<T, NV>(R, acc, slab, qj.f.N, qj.hr[j - 2], qj.own[j - 2]);
      }
    }
    plain_store_row<T, NV>(q.y + row, acc, slab);
    if (bn >= p.B) break;
    // this wave's DMA share landed: J >= 2 waited vmcnt(0) behind it; at J = 1 the 2 * NV coefficient stores
    // and the NV stores of y follow it
    wait_vmcnt<3 * NV>();
    cur = (cur + J) & 1;  // the buffer that was free during level J
    b = bn;
  }
}

// One kernel per (taps, accumulation mode); resident workgroups per CU from the occupancy API, as
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

template <int L, bool FMA>
static PairKernel* pair_kernel_of() {
  static PairKernel k;
  k.func = reinterpret_cast<const void*>(&k_roundtrip<double, L, FMA>);
  return &k;
}

static PairKernel* pair_kernel(int taps, bool fma) {
  switch (taps) {
#define VW_CASE(n) \
    case n:        \
      if constexpr (n <= kPairMaxTaps) return fma ? pair_kernel_of<n, true>() : pair_kernel_of<n, false>(); \
      break;
    VW_TAP_LIST(VW_CASE)
#undef VW_CASE
    default: break;
  }
  return nullptr;
}

// the dynamic-LDS limit of this device's copy of the kernel covers `lds` (set_lds)
static bool lds_ready(PairKernel* k, int lds) {
  if (lds <= 64 * 1024) return true;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return false;
  return k->lds.limit[dev].load(std::memory_order_acquire) >= lds;
}

hipError_t pair_prepare(int taps, bool fma, int threads, int lds, int* per_cu) {
  PairKernel* k = pair_kernel(taps, fma);
  if (!k) return hipErrorNotSupported;
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
  if (per_cu) *per_cu = n;
  return hipSuccess;
}

bool pair_launch_shape(int taps, bool fma, int threads, int lds, long long B, int cus, PairLaunch* out) {
  PairKernel* k = pair_kernel(taps, fma);
  if (!k || !lds_ready(k, lds)) return false;
  int n;
  {
    std::lock_guard<std::mutex> g(k->mu);
    n = k->find(threads, lds);
  }
  if (n < 1) return false;
  out->func = k->func;
  out->grid = (unsigned)std::min<long long>(B, (long long)n * cus);
  out->threads = (unsigned)threads;
  out->lds = (unsigned)lds;
  return true;
}

hipError_t launch_roundtrip(const PairArgs<double>& a, const PairLaunch& l, hipStream_t st) {
  void* params[] = {const_cast<PairArgs<double>*>(&a)};
  return hipLaunchKernel(l.func, dim3(l.grid), dim3(l.threads), params, l.lds, st);
}

}  // namespace vw
