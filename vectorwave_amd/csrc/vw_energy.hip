// vw_energy.hip -- wavelet energy per level: MultiLevelMODWTResult.getApproximationEnergy / getDetailEnergyAtLevel
// (core/modwt/MultiLevelMODWTResultImpl.java:91-117, computeEnergy :211-216) for a batch, on the device.
//
// Three kernel families:
//  * k_energy_fused (VW_FLAG_TREE_SUMS): k_forward_fused's cascade -- row to LDS with its halo, regs_to_level,
//    fwd_row with its unrolled tap bodies and compile-time strides -- whose emit squares and adds the outputs
//    instead of storing them.  x is read once, J+1 doubles per row are written, no coefficient goes to HBM.
//    Per level a thread keeps one partial; a wave butterfly folds it and lane 0 parks it in LDS; after the
//    last level J+1 threads add the waves' partials in wave order and store.  Fixed order: deterministic.
//  * k_energy_chain (default): the reference's `energy += c * c` in index order over planes in memory.  A
//    sequential fp64 chain per row, so one LANE per row and 64 rows per wave: the dependent v_add_f64 latency
//    is paid once per 64 rows.  Lanes of a wave own different rows (addresses N apart), so tiles of
//    [64 rows][kChainK elements] are staged through LDS: coalesced 16-byte global reads of row segments,
//    then each lane walks its own LDS row.  Rows are padded to kChainK + 2 doubles (68 dwords): lane l's
//    ds_read_b128 starts at bank 4l mod 64, conflict-free in every 16-lane group.  The next tile's loads
//    are in flight while the current one is walked.
//  * k_energy_rows_tree: planes in memory, VW_FLAG_TREE_SUMS: one workgroup per row, per-thread partials
//    and the fixed-order workgroup sum.
// Built with -ffp-contract=off: a square is rounded, then added.
#include "vw_launch_k.h"
#include "vw_dev_rows.h"

#include <algorithm>

namespace vw {

namespace {

// Wave sum in a fixed order (lane butterflies); every lane of a whole wave gets the total.
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Workgroup sum in a fixed order (lane butterflies, then the waves in order): every thread gets the total.
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double t = red[0];
  for (int k = 1; k < nw; ++k) t += red[k];
  return t;
}

}  // namespace

// One level of the cascade: the thread's sum of squared details; its approximations go to areg (the next
// level's input, or a_J).  Elements past the row add nothing.
template <int L, bool FMA, int NV>
__device__ __forceinline__ double energy_level(const EnergyArgs& p, const double* X, int nvec, const LevelDesc& lv,
                                               double (&areg)[NV][2]) {
  constexpr int V = 2;
  const int N = p.N;
  double ed = 0.0;
  fwd_row<double, L, FMA, NV>(X, nvec, lv.s, p.lo, p.hi, p.taps, p.level_ct,
                              [&](int k, int w, const double (&al)[V], const double (&ah)[V]) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (L > 0 || w * V + e < N) ed += ah[e] * ah[e];
      areg[k][e] = al[e];
    }
    // Pin the sums here (as inv_row_t): no store consumes this vector's outputs, and otherwise the arithmetic is
    // sunk past the next vectors' LDS reads, whose values then all stay live (VGPR spills).
    asm volatile("" : "+v"(ed));
#pragma unroll
    for (int e = 0; e < V; ++e) asm volatile("" : "+v"(areg[k][e]));
  });
  return ed;
}

// Host contract (vw_plan.cpp plan_energy): whole waves (blockDim.x a multiple of 64), the level buffers and
// kEnergyRed doubles at red_off within the dynamic LDS, no streaming history, no kHaloFftPad level.
// (6 waves per SIMD for the short filters' NV = 4 form: at the forward's 8 -- 64 VGPRs -- the running sum and its
// wave fold spill a few registers)
template <int L, bool FMA, int NV>
__global__ void VW_FUSED_BOUNDS(NV, VW_FUSED_W(L, 6)) k_energy_fused(const EnergyArgs p) {
  using T = double;
  constexpr int V = VT<T>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* const X0 = reinterpret_cast<T*>(smem) + p.hlpad;
  T* const Y0 = p.region1 ? X0 + p.region1 : X0;
  T* const red = reinterpret_cast<T*>(smem) + p.red_off;
  const bool dbl = p.region1 != 0;
  const int N = p.N;
  const int nvec = (N + V - 1) / V;
  const bool vec_ok = (L > 0) || p.vec_io != 0;  // unrolled kernels run with aligned rows only
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;

  for (long long b = blockIdx.x; b < p.B; b += gridDim.x) {
    T* X = X0;
    T* Y = Y0;
    T areg[NV][V];
    load_row_regs<T, NV>(areg, p.x + b * p.ldx, N, nvec, vec_ok, false);
    wait_vmem();
    regs_to_level<T, L, NV>(X, areg, nvec, N, p.lv[0], p.npow2, nullptr);
    for (int j = 1; j <= p.J; ++j) {
      const LevelDesc lv = p.lv[j - 1];
      lds_barrier();  // X = level input + halo; every read of Y (previous level) done
      const T ed = wave_sum(energy_level<L, FMA, NV>(p, X, nvec, lv, areg));
      if ((threadIdx.x & 63) == 0) red[j * kEnergyWaves + wave] = ed;
      if (j < p.J) {
        if (!dbl) lds_barrier();  // one buffer: every read of this level's input done first
        regs_to_level<T, L, NV>(Y, areg, nvec, N, p.lv[j], p.npow2, nullptr);
        T* t = X; X = Y; Y = t;
      }
    }
    // a_J is in the registers that would feed level J + 1
    T ea = T(0);
    for_vecs<L, NV>(nvec, [&](int k, int w) {
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (L > 0 || w * V + e < N) ea += areg[k][e] * areg[k][e];
    });
    ea = wave_sum(ea);
    if ((threadIdx.x & 63) == 0) red[wave] = ea;
    lds_barrier();  // the waves' partials are in LDS; every read of the level buffers done (the next row overwrites them)
    if ((int)threadIdx.x <= p.J) {
      const T* r = red + threadIdx.x * kEnergyWaves;
      T t = r[0];
      for (int k = 1; k < nw; ++k) t += r[k];
      p.out[(long long)threadIdx.x * p.B + b] = t;
    }
    // (the next row writes `red` only after its first level barrier, which these reads precede)
  }
}

hipError_t launch_energy_fused(const EnergyArgs& a, int threads, int lds, bool fma, int nv, int grid, hipStream_t st) {
  if (threads <= 0 || threads % 64 != 0 || grid <= 0 || (nv != 4 && nv != 8)) return hipErrorInvalidConfiguration;
  auto run = [&](auto l, auto m) {
    if (nv <= 4) return launch_k<k_energy_fused<l(), m(), 4>>(dim3((unsigned)grid), dim3(threads), lds, st, a);
    return launch_k<k_energy_fused<l(), m(), 8>>(dim3((unsigned)grid), dim3(threads), lds, st, a);
  };
  // Tap-unrolled bodies for the short filters only (kEnergyUnrollMax): under this kernel's register budget the
  // longer filters' unrolled windows spill to scratch, so they -- like unaligned rows and partial slabs -- take the
  // runtime-L body, which does not (plan_energy names no kernel this unit lacks).
  if (a.unrolled) return dispatch_taps<Unlisted::kInvalidConfiguration, kEnergyUnrollMax>(a.taps, fma, run);
  return with_fma(fma, [&](auto m) { return run(std::integral_constant<int, 0>{}, m); });
}

// ------------------------------------------------------------------------------------------------
// Planes in memory.

constexpr int kChainK = 32;                 // elements of a row per tile
constexpr int kChainStride = kChainK + 2;   // LDS row stride in doubles (see the header comment)
constexpr int kChainLoads = 64 * kChainK / 2 / 64;  // 16-byte loads per lane and tile: 16

typedef double vw_d2 __attribute__((ext_vector_type(2)));

// One wave per 64 rows of ONE array (approx: B rows, details: J*B rows; both N long and N apart), so a wave's
// rows are a uniform stride apart.  Workgroup g < ceil(B/64) walks approx rows, the others detail rows.
__global__ void __launch_bounds__(64) k_energy_chain(const EnergyPlanesArgs p) {
  __shared__ __attribute__((aligned(16))) double tile[64 * kChainStride];
  const int lane = threadIdx.x;
  const long long nwa = (p.B + 63) / 64;
  const bool is_a = (long long)blockIdx.x < nwa;
  const double* const arr = is_a ? p.approx : p.details;
  const long long nrows = is_a ? p.B : (long long)p.J * p.B;
  const long long r0 = ((long long)blockIdx.x - (is_a ? 0 : nwa)) * 64;
  const int N = p.N;
  const int sub = lane >> 4, l16 = lane & 15;
  const bool vec = p.vec_io != 0;

  // Loads only, unconditional: rows past the array re-read its last row, elements past the row re-read its
  // last ones; neither is ever walked.
  vw_d2 pf[kChainLoads];
  auto load_tile = [&](int i0) {
#pragma unroll
    for (int q = 0; q < kChainLoads; ++q) {
      const long long r = min(r0 + 4 * q + sub, nrows - 1);
      const double* const row = arr + r * (long long)N;
      const int e = i0 + 2 * l16;
      if (vec) {
        pf[q] = *reinterpret_cast<const vw_d2*>(row + min(e, N - 2));
      } else {
        pf[q][0] = row[min(e, N - 1)];
        pf[q][1] = row[min(e + 1, N - 1)];
      }
    }
  };

  const int ntiles = (N + kChainK - 1) / kChainK;
  const double* const mine = tile + lane * kChainStride;
  double acc = 0.0;
  load_tile(0);
  for (int t = 0; t < ntiles; ++t) {
    lds_barrier();  // (one wave: orders this tile's writes after the previous tile's reads)
#pragma unroll
    for (int q = 0; q < kChainLoads; ++q)
      *reinterpret_cast<vw_d2*>(tile + (4 * q + sub) * kChainStride + 2 * l16) = pf[q];
    load_tile(min(t + 1, ntiles - 1) * kChainK);  // the next tile (the last one again at the end: no branch)
    lds_barrier();
    const int kk = min(kChainK, N - t * kChainK);
    if (kk == kChainK) {
#pragma unroll
      for (int i = 0; i < kChainK; i += 2) {
        const vw_d2 v = *reinterpret_cast<const vw_d2*>(mine + i);
        acc += v[0] * v[0];
        acc += v[1] * v[1];
      }
    } else {
      for (int i = 0; i < kk; ++i) acc += mine[i] * mine[i];
    }
  }
  if (r0 + lane < nrows) p.out[(is_a ? 0 : p.B) + r0 + lane] = acc;
}

// VW_FLAG_TREE_SUMS over planes in memory: workgroup per row (approx rows, then detail rows: out[c] is row c).
__global__ void __launch_bounds__(256) k_energy_rows_tree(const EnergyPlanesArgs p) {
  __shared__ double red[4];
  const long long rows = ((long long)p.J + 1) * p.B;
  const int N = p.N, tid = threadIdx.x;
  for (long long c = blockIdx.x; c < rows; c += gridDim.x) {
    const double* const row = c < p.B ? p.approx + c * (long long)N : p.details + (c - p.B) * (long long)N;
    double s = 0.0;
    if (p.vec_io) {
      const vw_d2* const r2 = reinterpret_cast<const vw_d2*>(row);
#pragma unroll 4
      for (int i = tid; i < N / 2; i += 256) {
        const vw_d2 v = r2[i];
        s += v[0] * v[0];
        s += v[1] * v[1];
      }
    } else if (N % 2 == 0) {
      // rows that are not 16-byte aligned: the vector form's partial sums, element by element -- which terms a
      // thread adds, and in what order, must not depend on where the caller's arrays start
#pragma unroll 4
      for (int i = tid; i < N / 2; i += 256) {
        s += row[2 * i] * row[2 * i];
        s += row[2 * i + 1] * row[2 * i + 1];
      }
    } else {
#pragma unroll 4
      for (int i = tid; i < N; i += 256) s += row[i] * row[i];
    }
    const double t = block_sum(s, red);
    if (tid == 0) p.out[c] = t;
  }
}

hipError_t launch_energy_planes(const EnergyPlanesArgs& a, bool tree, int cus, hipStream_t st) {
  if (a.B <= 0 || a.N <= 0 || a.J < 0 || (a.vec_io && a.N % 2 != 0)) return hipErrorInvalidValue;
  if (tree) {
    const long long rows = ((long long)a.J + 1) * a.B;
    const long long grid = std::min<long long>(rows, 8LL * std::max(cus, 1));
    return launch_k<k_energy_rows_tree>(dim3((unsigned)grid), dim3(256), 0, st, a);
  } else {
    const long long grid = (a.B + 63) / 64 + ((long long)a.J * a.B + 63) / 64;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    return launch_k<k_energy_chain>(dim3((unsigned)grid), dim3(64), 0, st, a);
  }
}

}  // namespace vw
