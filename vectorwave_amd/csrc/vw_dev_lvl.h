#pragma once
// vw_dev_lvl.h -- the per-level path of signals too long for the fused kernels: the tiled level kernels
// (k_forward_level / k_inverse_level), the column sweeps (k_*_sweep, k_inverse_sweep2 / 3) and the multi-level
// tiles (k_*_multi; k_inverse_multi borrows vw_blk.h's BlkC).  Launched by vw_lvl.hip.
#include "vw_blk.h"

#pragma clang fp contract(off)

namespace vw {

// ---------------------------------------------------------------------------------------------
// Per-level tiled kernels (signals longer than the fused kernels hold in LDS).  One workgroup per
// (tile, signal); the tile and its halo are gathered from HBM through the reference's index map.
template <typename T>
__device__ __forceinline__ T halo_value_global(const T* __restrict__ src, int idx, int N, int mode, int npow2,
                                               const T* hist_b, int hist_len) {
  if (idx >= 0 && idx < N) return src[idx];
  switch (mode) {
    case kHaloPeriodic: { int r = idx % N; if (r < 0) r += N; return src[r]; }
    case kHaloSymmetric: return src[sym_index(idx, N)];
    case kHaloFftPad: { int r = idx < 0 ? idx + npow2 : idx; return (r >= 0 && r < N) ? src[r] : T(0); }
    case kHaloHistory: return (idx < 0 && idx >= -hist_len) ? hist_b[hist_len + idx] : T(0);
    default: return T(0);
  }
}

template <typename T>
__device__ __forceinline__ void tile_to_lds(T* buf, const T* __restrict__ src, int N, int ts, int lo_q, int hi_q,
                                            int mode, int npow2, const T* hist_b, int hist_len, const T* thr,
                                            T thr_b, int soft, bool zero, bool vec_ok = false) {
  // buf[q] = value at signal index ts + q, q in [lo_q, hi_q).  The in-range middle moves as 16-byte
  // vectors (ts and the vector bounds are multiples of V; rows 16-B aligned when vec_ok); the
  // ends go through the index map element by element.
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  int qa = lo_q, qb = lo_q;  // vector range [qa, qb)
  if (vec_ok && !zero) {
    qa = max(lo_q, -ts);
    qa = (qa + V - 1) / V * V;
    qb = min(hi_q, N - ts);
    qb = qb >= qa ? qa + (qb - qa) / V * V : qa;
  }
  for (int q = qa + (int)threadIdx.x * V; q < qb; q += blockDim.x * V) {
    vec v = __builtin_nontemporal_load(reinterpret_cast<const vec*>(src + ts + q));
    if (thr) {
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = threshold_t(v[e], thr_b, soft);
    }
    *reinterpret_cast<vec*>(buf + q) = v;
  }
  const int tail = (hi_q - lo_q) - (qb - qa);
  for (int r = (int)threadIdx.x; r < tail; r += blockDim.x) {
    const int q = (lo_q + r < qa) ? lo_q + r : qb + (r - (qa - lo_q));
    T v = zero ? T(0) : halo_value_global(src, ts + q, N, mode, npow2, hist_b, hist_len);
    if (thr) v = threshold_t(v, thr_b, soft);
    buf[q] = v;
  }
}

template <typename T, int L, bool FMA>
__global__ void __launch_bounds__(256) k_forward_level(const LevelArgs<T> p) {
  constexpr int V = VT<T>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* buf = reinterpret_cast<T*>(smem) + p.hlpad;
  const long long b = blockIdx.y;
  const int N = p.N;
  const int ts = blockIdx.x * p.tile;
  const int cnt = min(p.tile, N - ts);
  const int nv = (cnt + V - 1) / V;
  const LevelDesc lv = p.lv;
  const T* src = p.src_a + b * p.lda;
  const T* hist_b = (lv.mode == kHaloHistory) ? p.hist + b * lv.hist_len : nullptr;
  tile_to_lds(buf, src, N, ts, -lv.hl, nv * V, lv.mode, p.npow2, hist_b, lv.hist_len, (const T*)nullptr, T(0), 0,
              false, p.vec_io != 0 && (p.lda % V) == 0);
  if (p.validate) {
    for (int q = threadIdx.x; q < cnt; q += blockDim.x)
      if (!finite_t(buf[q])) atomicMin(p.bad, (unsigned long long)b * N + ts + q);
  }
  __syncthreads();
  const bool vec_ok = p.vec_io != 0;  // rows 16-B aligned (tile starts are multiples of V)
  for (int w = threadIdx.x; w < nv; w += blockDim.x) {
    const int t0 = w * V;
    T al[V], ah[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { al[e] = T(0); ah[e] = T(0); }
    fwd_vec<T, L, FMA>(buf, t0, lv.s, p.lo, p.hi, p.taps, al, ah);
    store_vec(p.out_a + b * (size_t)N + ts, t0, cnt, vec_ok, al);
    store_vec(p.out_d + b * (size_t)N + ts, t0, cnt, vec_ok, ah);
    check_out<T>(p.validate, p.bad, (unsigned long long)b * N + ts, t0, cnt, al);
    check_out<T>(p.validate, p.bad, (unsigned long long)b * N + ts, t0, cnt, ah);
  }
}

template <typename T, int L, bool FMA>
__global__ void __launch_bounds__(256) k_inverse_level(const LevelArgs<T> p) {
  constexpr int V = VT<T>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* A = reinterpret_cast<T*>(smem) + p.hlpad;
  T* D = reinterpret_cast<T*>(smem) + p.region_d + p.hlpad_d;
  const long long b = blockIdx.y;
  const int N = p.N;
  const int ts = blockIdx.x * p.tile;
  const int cnt = min(p.tile, N - ts);
  const int nv = (cnt + V - 1) / V;
  const LevelDesc lv = p.lv;
  const T thr_b = p.thr ? p.thr[b] : T(0);  // this launch is one level: the host offsets thr
  const int span = nv * V;
  tile_to_lds(A, p.src_a + b * (size_t)N, N, ts, -lv.hl, span + lv.hr, lv.mode, 0, (const T*)nullptr, 0,
              (const T*)nullptr, T(0), 0, p.src_a == nullptr, p.vec_io != 0);
  tile_to_lds(D, p.src_d + b * (size_t)N, N, ts, -lv.hl, span + lv.hr, lv.mode, 0, (const T*)nullptr, 0, p.thr,
              thr_b, p.soft, p.use_d == 0 || p.src_d == nullptr, p.vec_io != 0);
  __syncthreads();
  const bool vec_ok = p.vec_io != 0;
  for (int w = threadIdx.x; w < nv; w += blockDim.x) {
    const int t0 = w * V;
    T acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = T(0);
    if (p.pair) {
      inv_pair<T, L, FMA>(A, D, t0, lv.s, lv.dir_a, p.lo, p.hi, p.taps, acc);
    } else {
      inv_branch<T, L, FMA>(A, t0, lv.s, lv.dir_a, lv.off_a, p.lo, p.taps, acc);
      inv_branch<T, L, FMA>(D, t0, lv.s, lv.dir_d, lv.off_d, p.hi, p.taps, acc);
    }
    store_vec(p.out_a + b * (size_t)N + ts, t0, cnt, vec_ok, acc);
  }
}

// ---------------------------------------------------------------------------------------------
// Column-sweep kernels for deep levels of long signals (spacing s >= kSweepMinS).  At spacing s
// the level's convolution never mixes residues mod s: view the row as a matrix [N/s][s] and every
// column r is an independent dense L-tap filter over q (t = r + q*s).  One thread owns one column
// and a chunk of QC consecutive q, keeping the L most recent inputs in a register window: each
// input is read from HBM once (+ L-1 warm-up reads per chunk), lanes read consecutive residues
// (>= 128 contiguous bytes per lane group), and there is no LDS halo -- which at level 10 of db8
// (15 x 512 = 7,680 samples) tripled the tiled kernel's reads.  Elements outside [0, N) (warm-up,
// wrap, tail) go through the reference's index map (halo_value_global), so every boundary mode and
// any N (wraps that change residue when s does not divide N) is exact; summation order per output
// is the reference's (taps ascending; approximation branch, then detail branch).
// kSweepMinS (vw_internal.h) = 16: 16 x 8 B = 128 B contiguous per lane group (fp64).

struct SweepPos {
  long long b;
  int r, q0, q1;  // column r, q in [q0, q1)
  bool ok;
};

__device__ __forceinline__ SweepPos sweep_pos(long long B, int N, int s, int qc) {
  // thread -> (signal, chunk, residue), residue fastest: consecutive lanes = consecutive addresses
  const int qn = (N + s - 1) / s;  // q extent of column 0
  const int chunks = (qn + qc - 1) / qc;
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per = (long long)chunks * s;
  SweepPos p;
  p.b = g / per;
  const long long rem = g - p.b * per;
  const int c = (int)(rem / s);
  p.r = (int)(rem - (long long)c * s);
  const int qr = p.r < N ? (N - 1 - p.r) / s + 1 : 0;  // column r length
  p.q0 = c * qc;
  p.q1 = min(p.q0 + qc, qr);
  p.ok = p.b < B && p.q0 < p.q1;
  return p;
}

template <typename T>
__device__ __forceinline__ T sweep_fetch(const T* __restrict__ src, long long u, int N, int mode, int npow2,
                                         const T* hist_b, int hist_len) {
  if (u >= 0 && u < N) return src[u];
  return halo_value_global(src, (int)u, N, mode, npow2, hist_b, hist_len);
}

// Register window of one branch over a block of K outputs t_k = t_b + k*s (k < K):
//   DIR = -1 (reads t - i*s + off):  w[j] = value at t_b + off + (j - (L-1))*s, tap i of output k = w[k - i + L - 1]
//   DIR = +1 (reads t + i*s + off):  w[j] = value at t_b + off + j*s,           tap i of output k = w[k + i]
// j in [0, K + L - 1).  Between blocks the last L - 1 values move to the front and K new values are
// loaded -- all K loads of a block in flight at once (one load per output step would expose the
// full memory latency per output).
template <typename T, int L, int K, int DIR>
struct SweepWin {
  T w[K + L - 1];
  __device__ __forceinline__ long long first(long long tb, int s, int off) const {
    return tb + off + (DIR < 0 ? -(long long)(L - 1) * s : 0);
  }
  template <typename Fetch>
  __device__ __forceinline__ void fill_head(long long tb, int s, int off, Fetch&& fetch) {  // j < L - 1
    const long long u0 = first(tb, s, off);
#pragma unroll
    for (int j = 0; j < L - 1; ++j) w[j] = fetch(u0 + (long long)j * s);
  }
  template <typename Fetch>
  __device__ __forceinline__ void load_block(long long tb, int s, int off, Fetch&& fetch) {  // j >= L - 1
    const long long u0 = first(tb, s, off);
#pragma unroll
    for (int j = L - 1; j < K + L - 1; ++j) w[j] = fetch(u0 + (long long)j * s);
  }
  __device__ __forceinline__ void shift() {
#pragma unroll
    for (int j = 0; j < L - 1; ++j) w[j] = w[j + K];
  }
  __device__ __forceinline__ T tap(int k, int i) const { return DIR < 0 ? w[k - i + L - 1] : w[k + i]; }
};

// outputs per register block (loads in flight per branch); long filters keep their windows in budget
template <int L> struct SweepK { static constexpr int K = L <= 16 ? 16 : 8; };

// Forward, one level: a[t] = sum_i lo[i] x[g(t - i s)], d[t] likewise (ScalarOps.java:700-835 order).
template <typename T, int L, bool FMA>
__global__ void __launch_bounds__(256) k_forward_sweep(const LevelArgs<T> p) {
  constexpr int K = SweepK<L>::K;
  const LevelDesc lv = p.lv;
  const int s = lv.s, N = p.N;
  const SweepPos sp = sweep_pos(p.B, N, s, p.tile);
  if (!sp.ok) return;
  const T* src = p.src_a + sp.b * p.lda;
  const T* hist_b = (lv.mode == kHaloHistory) ? p.hist + sp.b * lv.hist_len : nullptr;
  T* oa = p.out_a + sp.b * (size_t)N;
  T* od = p.out_d + sp.b * (size_t)N;
  const unsigned long long flat0 = (unsigned long long)sp.b * N;
  // inputs at or beyond the column end are never used by a stored output: read them as zero
  const long long tend = (long long)sp.r + (long long)sp.q1 * s;
  auto fetch = [&](long long u) -> T {
    if (u >= tend) return T(0);
    return sweep_fetch(src, u, N, lv.mode, p.npow2, hist_b, lv.hist_len);
  };
  SweepWin<T, L, K, -1> X;
  long long tb = (long long)sp.r + (long long)sp.q0 * s;
  X.fill_head(tb, s, 0, fetch);
  for (int q = sp.q0; q < sp.q1; q += K, tb += (long long)K * s) {
    X.load_block(tb, s, 0, fetch);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (q + k < sp.q1) {
        T al = T(0), ah = T(0);
#pragma unroll
        for (int i = 0; i < L; ++i) {
          al = madd<FMA>(al, X.tap(k, i), p.lo[i]);
          ah = madd<FMA>(ah, X.tap(k, i), p.hi[i]);
        }
        const long long t = tb + (long long)k * s;
        oa[t] = al;
        od[t] = ah;
        if (p.validate) {
          if (!finite_t(X.tap(k, 0))) atomicMin(p.bad, flat0 + t);
          if (!finite_t(al) || !finite_t(ah)) atomicMin(p.bad, (1ull << 62) | (flat0 + t));
        }
      }
    }
    X.shift();
  }
}

// Inverse, one level: approximation branch (lo, dir_a, off_a) and detail branch (hi, dir_d, off_d),
// each its own register window; sums in the reference's order (K4/K6 sequential, K5 pairwise).
template <typename T, int L, bool FMA, int DA, int DD>
__global__ void __launch_bounds__(256) k_inverse_sweep(const LevelArgs<T> p) {
  constexpr int K = SweepK<L>::K;
  const LevelDesc lv = p.lv;
  const int s = lv.s, N = p.N;
  const SweepPos sp = sweep_pos(p.B, N, s, p.tile);
  if (!sp.ok) return;
  const T thr_b = p.thr ? p.thr[sp.b] : T(0);
  const T* sa = p.src_a ? p.src_a + sp.b * (size_t)N : nullptr;
  const T* sd = p.src_d ? p.src_d + sp.b * (size_t)N : nullptr;
  const bool za = sa == nullptr, zd = sd == nullptr || p.use_d == 0;
  T* y = p.out_a + sp.b * (size_t)N;
  auto fa = [&](long long u) -> T { return za ? T(0) : sweep_fetch(sa, u, N, lv.mode, 0, (const T*)nullptr, 0); };
  auto fd = [&](long long u) -> T {
    if (zd) return T(0);
    const T v = sweep_fetch(sd, u, N, lv.mode, 0, (const T*)nullptr, 0);
    return p.thr ? threshold_t(v, thr_b, p.soft) : v;
  };
  SweepWin<T, L, K, DA> A;
  SweepWin<T, L, K, DD> D;
  long long tb = (long long)sp.r + (long long)sp.q0 * s;
  A.fill_head(tb, s, lv.off_a, fa);
  D.fill_head(tb, s, lv.off_d, fd);
  for (int q = sp.q0; q < sp.q1; q += K, tb += (long long)K * s) {
    A.load_block(tb, s, lv.off_a, fa);
    D.load_block(tb, s, lv.off_d, fd);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (q + k < sp.q1) {
        T acc = T(0);
        if (p.pair) {  // MODWTTransform.inverse / K5: sum += h*a + g*d per tap
#pragma unroll
          for (int i = 0; i < L; ++i) acc = acc + pair_term<T, FMA>(p.lo[i], A.tap(k, i), p.hi[i], D.tap(k, i));
        } else {       // K4 / K6: all approximation taps, then all detail taps
#pragma unroll
          for (int i = 0; i < L; ++i) acc = madd<FMA>(acc, A.tap(k, i), p.lo[i]);
#pragma unroll
          for (int i = 0; i < L; ++i) acc = madd<FMA>(acc, D.tap(k, i), p.hi[i]);
        }
        y[tb + (long long)k * s] = acc;
      }
    }
    A.shift();
    D.shift();
  }
}

// ---------------------------------------------------------------------------------------------
// Two or three inverse levels per launch: levels j, j-1 (, j-2) with spacings G*h .. h (G = 2 or 4),
// PERIODIC, sequential sums (K4: MultiLevelMODWTTransform.java:576-589), as column sweeps chained
// through LDS rings, so the intermediate approximations never go to HBM (4 rows per pair of levels
// instead of 6, 5 per triple instead of 9).
//
// In the residue class r mod h, position u is the sample t = r + u*h (u < nu = N/h); the bottom level
// reads u + i, the one above u + 2i, the top u + G*i -- so the top level is a plain sweep over each of
// the G classes u = G*v + e (r + e*h mod G*h).  A workgroup owns R consecutive residues (R = 64: one
// fp64 per lane, 512 contiguous bytes per wave access; R = 32 where h = 32: two residue groups per
// wave, 256 B each) of one signal and a chunk [u0, u1) of u, in groups of R threads:
//   top groups (G of them): group e sweeps class e of the top level with register windows (as
//     k_inverse_sweep) and writes its KA outputs of block n (KB = G*KA positions) into ring 1 at step n;
//   middle groups (triple, 4): at step n, level j-1 over block n-2 -- parity e2, half of the parity's
//     2*KA outputs -- reading a_{j-1}[u + 2i] from ring 1 (it reaches into block n-1, complete) and
//     d_{j-1} from HBM, writing a_{j-2} into ring 2;
//   bottom groups (4 of a triple, 2 of a pair): at step 2 (pair) / 4 (triple) behind the top, KA
//     outputs of the bottom level each, ring -> y in HBM.
// One barrier per step; every ring holds three blocks.  The upper stages run past the chunk by their
// reach (L-1 positions at each level below, <= KB) and wrap mod N: every value equals the reference's
// (t+l)%N read, products summed in the same order -> bit-exact in EXACT mode.
// Host contract (vw_plan.cpp sweepg_plan): h % R == 0, N % (G*h) == 0, every level PERIODIC / dir +1 / offset 0,
// (2*KB + 2*L) * G*h <= N (one wrap at most), KB >= 2*(L-1), p.tile (u per chunk) a multiple of KB.

// KA outputs of one level at u = ub + st*k (k < KA, st = the level's spacing in u): a from an LDS ring
// (slot of ub: sl0, slot stride st), d from HBM at t = tb + x*ts (ts = st*h); the approximation branch,
// then the detail branch, each i ascending.
template <typename T, int L, bool FMA, int KA, int R, int RING>
__device__ __forceinline__ void sweep_ring_stage(const T* ring, int lane, int sl0, int st, const T* sd, bool thr_on,
                                                 T thr_b, int soft, long long tb, long long ts, int N, const T* lo,
                                                 const T* hi, T (&acc)[KA]) {
  T wd[KA + L - 1];
#pragma unroll
  for (int x = 0; x < KA + L - 1; ++x) {  // issued first: in flight during the approximation branch
    if (sd) {
      long long t = tb + (long long)x * ts;
      t = t >= N ? t - N : t;
      const T v = sd[t];
      wd[x] = thr_on ? threshold_t(v, thr_b, soft) : v;
    } else {
      wd[x] = T(0);
    }
  }
  T w[KA + L - 1];
#pragma unroll
  for (int x = 0; x < KA + L - 1; ++x) {
    const int sl = sl0 + x * st;
    w[x] = ring[(sl >= RING ? sl - RING : sl) * R + lane];
  }
#pragma unroll
  for (int k = 0; k < KA; ++k) {
    acc[k] = T(0);
#pragma unroll
    for (int i = 0; i < L; ++i) acc[k] = madd<FMA>(acc[k], w[k + i], lo[i]);
  }
#pragma unroll
  for (int k = 0; k < KA; ++k)
#pragma unroll
    for (int i = 0; i < L; ++i) acc[k] = madd<FMA>(acc[k], wd[k + i], hi[i]);
}

// Workgroup -> (signal, R-residue block, u-chunk)
struct SweepGPos {
  long long b;
  int r0, u0, u1;
};
__device__ __forceinline__ bool sweepg_pos(long long B, int N, int h, int R, int uc, SweepGPos* w) {
  const int nu = N / h, nrb = h / R, nch = (nu + uc - 1) / uc;
  long long id = blockIdx.x;
  const int ch = (int)(id % nch);
  id /= nch;
  w->r0 = (int)(id % nrb) * R;
  w->b = id / nrb;
  w->u0 = ch * uc;
  w->u1 = min(w->u0 + uc, nu);
  return w->b < B;
}

// Top stage, class e of G: level-j sweep over t = r + e*h + v*G*h; one step writes KA outputs.
template <typename T, int L, bool FMA, int KA>
struct SweepTop {
  SweepWin<T, L, KA, 1> A, D;
  long long tb;
  int S, N;
  const T *sa, *sd;
  bool thr_on;
  T thr_b;
  int soft;
  __device__ __forceinline__ T fa(long long t) const { return sa ? sa[t >= N ? t - N : t] : T(0); }
  __device__ __forceinline__ T fd(long long t) const {
    if (!sd) return T(0);
    const T v = sd[t >= N ? t - N : t];
    return thr_on ? threshold_t(v, thr_b, soft) : v;
  }
  __device__ __forceinline__ void start() {
    A.fill_head(tb, S, 0, [&](long long t) { return fa(t); });
    D.fill_head(tb, S, 0, [&](long long t) { return fd(t); });
  }
  template <typename Out>
  __device__ __forceinline__ void step(const T* lo, const T* hi, Out&& out) {
    A.load_block(tb, S, 0, [&](long long t) { return fa(t); });
    D.load_block(tb, S, 0, [&](long long t) { return fd(t); });
#pragma unroll
    for (int k = 0; k < KA; ++k) {
      T acc = T(0);
#pragma unroll
      for (int i = 0; i < L; ++i) acc = madd<FMA>(acc, A.tap(k, i), lo[i]);
#pragma unroll
      for (int i = 0; i < L; ++i) acc = madd<FMA>(acc, D.tap(k, i), hi[i]);
      out(k, acc);
    }
    A.shift();
    D.shift();
    tb += (long long)KA * S;
  }
};

// Pair (G = 2): groups 0, 1 top (parity), 2, 3 bottom (half of a block).
template <typename T, int L, bool FMA, int KA, int R>
__global__ void __launch_bounds__(4 * R) k_inverse_sweep2(const LevelArgs<T> p) {
  constexpr int KB = 2 * KA;
  constexpr int RING = 3 * KB;
  static_assert(KB >= L - 1, "the bottom level reads at most one block ahead");
  __shared__ T ring[RING * R];
  const int S = p.lv.s, h = S >> 1, N = p.N;
  SweepGPos w;
  if (!sweepg_pos(p.B, N, h, R, p.tile, &w)) return;  // workgroup-uniform
  const int g = threadIdx.x / R, lane = threadIdx.x % R;
  const int r = w.r0 + lane;
  const int nblk = (w.u1 - w.u0 + KB - 1) / KB;
  const size_t row = (size_t)w.b * (size_t)N;
  if (g < 2) {
    SweepTop<T, L, FMA, KA> top;
    top.S = S; top.N = N; top.soft = p.soft;
    top.sa = p.src_a ? p.src_a + row : nullptr;
    top.sd = (p.src_d && p.use_d) ? p.src_d + row : nullptr;
    top.thr_on = p.thr != nullptr;
    top.thr_b = p.thr ? p.thr[w.b] : T(0);
    top.tb = (long long)r + (long long)g * h + (long long)(w.u0 >> 1) * S;
    top.start();
    for (int n = 0; n <= nblk + 1; ++n) {
      if (n <= nblk) {
        T* rn = ring + ((n % 3) * KB + g) * R + lane;
        top.step(p.lo, p.hi, [&](int k, T v) { rn[2 * k * R] = v; });  // u = u0 + n*KB + 2k + g
      }
      __syncthreads();
    }
  } else {
    const int hh = g - 2;
    const T* sd = (p.src_d2 && p.use_d2) ? p.src_d2 + row : nullptr;
    const T thr_b = p.thr2 ? p.thr2[w.b] : T(0);
    T* y = p.out_a + row;
    for (int n = 0; n <= nblk + 1; ++n) {
      if (n >= 2) {
        const int m = n - 2;
        const int ub = w.u0 + m * KB + hh * KA;
        T acc[KA];
        sweep_ring_stage<T, L, FMA, KA, R, RING>(ring, lane, (m % 3) * KB + hh * KA, 1, sd, p.thr2 != nullptr, thr_b,
                                                 p.soft, (long long)r + (long long)ub * h, h, N, p.lo, p.hi, acc);
#pragma unroll
        for (int k = 0; k < KA; ++k)
          if (ub + k < w.u1) y[(size_t)r + (size_t)(ub + k) * (size_t)h] = acc[k];
      }
      __syncthreads();
    }
  }
}

// Triple (G = 4): groups 0..3 top (class u mod 4), 4..7 middle (parity, half), 8..11 bottom (quarter).
template <typename T, int L, bool FMA, int KA, int R>
__global__ void __launch_bounds__(12 * R) k_inverse_sweep3(const LevelArgs<T> p) {
  constexpr int KB = 4 * KA;
  constexpr int RING = 3 * KB;
  static_assert(KB >= 2 * (L - 1), "the middle level reads at most one block ahead");
  __shared__ T ring1[RING * R];
  __shared__ T ring2[RING * R];
  const int S = p.lv.s, h = S >> 2, N = p.N;
  SweepGPos w;
  if (!sweepg_pos(p.B, N, h, R, p.tile, &w)) return;  // workgroup-uniform
  const int g = threadIdx.x / R, lane = threadIdx.x % R;
  const int r = w.r0 + lane;
  const int nblk = (w.u1 - w.u0 + KB - 1) / KB;
  const size_t row = (size_t)w.b * (size_t)N;
  // top: blocks 0 .. nblk+1 at steps n; middle: blocks 0 .. nblk at n-2; bottom: blocks 0 .. nblk-1 at n-4
  if (g < 4) {
    SweepTop<T, L, FMA, KA> top;
    top.S = S; top.N = N; top.soft = p.soft;
    top.sa = p.src_a ? p.src_a + row : nullptr;
    top.sd = (p.src_d && p.use_d) ? p.src_d + row : nullptr;
    top.thr_on = p.thr != nullptr;
    top.thr_b = p.thr ? p.thr[w.b] : T(0);
    top.tb = (long long)r + (long long)g * h + (long long)(w.u0 >> 2) * S;
    top.start();
    for (int n = 0; n <= nblk + 3; ++n) {
      if (n <= nblk + 1) {
        T* rn = ring1 + ((n % 3) * KB + g) * R + lane;
        top.step(p.lo, p.hi, [&](int k, T v) { rn[4 * k * R] = v; });  // u = u0 + n*KB + 4k + g
      }
      __syncthreads();
    }
  } else if (g < 8) {
    const int e2 = (g - 4) & 1, half = (g - 4) >> 1;
    const T* sd = (p.src_d2 && p.use_d2) ? p.src_d2 + row : nullptr;
    const T thr_b = p.thr2 ? p.thr2[w.b] : T(0);
    for (int n = 0; n <= nblk + 3; ++n) {
      if (n >= 2 && n <= nblk + 2) {
        const int m = n - 2;
        const int o = e2 + 2 * half * KA;  // u offset of this group's first output in the block
        const int ub = w.u0 + m * KB + o;
        T acc[KA];
        sweep_ring_stage<T, L, FMA, KA, R, RING>(ring1, lane, (m % 3) * KB + o, 2, sd, p.thr2 != nullptr, thr_b, p.soft,
                                                 (long long)r + (long long)ub * h, 2LL * h, N, p.lo, p.hi, acc);
        T* rn = ring2 + ((m % 3) * KB + o) * R + lane;
#pragma unroll
        for (int k = 0; k < KA; ++k) rn[2 * k * R] = acc[k];
      }
      __syncthreads();
    }
  } else {
    const int q = g - 8;
    const T* sd = (p.src_d3 && p.use_d3) ? p.src_d3 + row : nullptr;
    const T thr_b = p.thr3 ? p.thr3[w.b] : T(0);
    T* y = p.out_a + row;
    for (int n = 0; n <= nblk + 3; ++n) {
      if (n >= 4) {
        const int m = n - 4;
        const int ub = w.u0 + m * KB + q * KA;
        T acc[KA];
        sweep_ring_stage<T, L, FMA, KA, R, RING>(ring2, lane, (m % 3) * KB + q * KA, 1, sd, p.thr3 != nullptr, thr_b,
                                                 p.soft, (long long)r + (long long)ub * h, h, N, p.lo, p.hi, acc);
#pragma unroll
        for (int k = 0; k < KA; ++k)
          if (ub + k < w.u1) y[(size_t)r + (size_t)(ub + k) * (size_t)h] = acc[k];
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Multi-level tiles for long PERIODIC signals (host: vw_plan.cpp level_groups).  One workgroup runs
// a group of consecutive levels over one tile of one signal; the intermediate approximations stay
// in LDS.  Periodic convolution commutes with shifts, so a level evaluated at a position v outside
// [0, N) (the tile's halo) equals the reference's value at v mod N bit for bit -- the same products
// summed in the same order -- and only the group's inputs go through the index map.  Each level is
// evaluated over the tile plus the reach of the levels after it: to the left in the forward
// (ScalarOps.java:700-723 reads t - l*s), to the right in the inverse (MultiLevelMODWTTransform
// .java:576-589 reads t + l*s).  The redundant ext/tile of the arithmetic buys one HBM round trip
// per group instead of one per level.
template <typename T, int L, bool FMA>
__global__ void __launch_bounds__(256) k_forward_multi(const MultiArgs<T> p) {
  constexpr int V = VT<T>::V;
  using vec = typename VT<T>::v;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* X = reinterpret_cast<T*>(smem) + p.ext[0];  // level input, positions [-ext[k], span)
  T* Y = X + p.region;
  const long long b = blockIdx.y;
  const int N = p.N;
  const int ts = blockIdx.x * p.tile;
  const int cnt = min(p.tile, N - ts);
  const int span = (cnt + V - 1) / V * V;
  tile_to_lds(X, p.src_a + b * p.lda, N, ts, -p.ext[0], span, kHaloPeriodic, 0, (const T*)nullptr, 0,
              (const T*)nullptr, T(0), 0, false, p.vec_io != 0);
  const bool vec_ok = p.vec_io != 0;
  for (int k = 0; k < p.nlev; ++k) {
    lds_barrier();  // X complete; every read of Y (the previous level's input) done
    const int s = p.s0 << k;
    const int q_lo = -p.ext[k + 1];  // outputs [q_lo, span): the tile + what the next levels read
    const int nv = (span - q_lo) / V;
    const bool last = k == p.nlev - 1;
    T* od = p.out_d[k] + b * (size_t)N + ts;
    T* oa = p.out_a + b * (size_t)N + ts;
    for (int w = threadIdx.x; w < nv; w += blockDim.x) {
      const int q0 = q_lo + w * V;
      T al[V], ah[V];
#pragma unroll
      for (int e = 0; e < V; ++e) { al[e] = T(0); ah[e] = T(0); }
      fwd_vec<T, L, FMA>(X, q0, s, p.lo, p.hi, p.taps, al, ah);
      if (q0 >= 0) {  // the tile's own outputs (vectors never straddle 0: q_lo is a multiple of V)
        store_vec(od, q0, cnt, vec_ok, ah);
        if (last) store_vec(oa, q0, cnt, vec_ok, al);
      }
      if (!last) {
        vec o;
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = al[e];
        *reinterpret_cast<vec*>(Y + q0) = o;
      }
    }
    T* t = X; X = Y; Y = t;
  }
}

// Inverse: A = a_j, D = d_j (thresholded on load for denoise); a_{j-1} is computed into registers
// (NI vectors per thread) and written over A after a barrier -- two LDS regions, so three 256-thread
// workgroups fit a CU (a third region for a_{j-1} measured 1.2x slower: two per CU).  NI = 4 (fp64, host
// policy) on a tile whose register-blocked levels give all four waves work: at NI = 8 a 2048-sample db8
// tile had 129-144 threads of work per level, one SIMD idle and one mostly idle.
template <typename T, int L, bool FMA, int NI = kMultiInvNI>
__global__ void __launch_bounds__(256) k_inverse_multi(const MultiArgs<T> p) {
  constexpr int V = VT<T>::V;
  static_assert(NI == 8 || NI == 4, "outputs per thread");  // host contract: every level's blocks fit 256 threads
  using vec = typename VT<T>::v;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* const A = reinterpret_cast<T*>(smem);  // positions [0, span + ext[k])
  T* const D = A + p.region;
  const long long b = blockIdx.y;
  const int N = p.N;
  const int ts = blockIdx.x * p.tile;
  const int cnt = min(p.tile, N - ts);
  const int span = (cnt + V - 1) / V * V;
  const bool vec_ok = p.vec_io != 0;
  const int top = p.nlev - 1;
  T nf = T(0);  // VW_FLAG_REF_NONFINITE (p.nf_flag: the group ends at level 1): y's probe
  // Detail prefetch (p.pf, host contract: whole vectors, (span + ext[top]) / V <= kMultiPF * 256): the
  // tile of d_{k-1} is loaded into registers right after level k's first barrier and written to D
  // after its second, so the HBM latency of the next level's input overlaps this level's arithmetic.
  // The loads are unconditional (clamped vector index): an exec-masked load block makes the waitcnt
  // pass wait for it at the first LDS read.
  const bool pf = p.pf != 0;
  // Padded LDS layout (p.pad, host contract: pf and rblk on): the register-blocked levels (vector
  // stride m = s/V in 1..8) read lanes NI*m vectors apart -- an 8-way bank conflict at m = 1 in the
  // natural layout (62 % of LDS cycles in conflicts on db8 levels 1-5, profiles/r03/pmc_db8_stream.txt).
  // Level k's A and D then hold logical vector u at u + u/8 at NI = 8, at NI = 4 at u + u/4
  // (m <= 4) or u + 2*(u/8) (m = 8) -- blk_pad's NV = 8 / NV = 4 layouts, conflict-free ds_read_b128 at every
  // m <= 8 under the gfx950 lane groups; levels with m = 0 or m >= 16 keep the natural layout.
  // (a layout is (shift, pad): u -> u + (u >> shift) * pad -- one formula, no per-layout copies of the
  // hoisted store addresses)
  // The rule is blk_pad (vw_internal.h), restated: through blk_pad this run-time form compiled to other code.
  auto layout = [&](int k) {
    const int sk = p.s0 << k, m = sk / V;
    int2 lay = make_int2(30, 0);
    if (p.pad != 0 && sk >= V && sk % V == 0) {
      if constexpr (NI >= 8) {
        if (m < 16) lay = make_int2(3, 1);
      } else {
        if (m <= 4) lay = make_int2(2, 1);
        else if (m == 8) lay = make_int2(3, 2);
      }
    }
    return lay;
  };
  auto padded = [](int2 lay) { return lay.y != 0; };
  auto phys = [](int u, int2 lay) { return u + (u >> lay.x) * lay.y; };
  vec dreg[kMultiPF];
  auto d_load = [&](int k) {
    const T* sd = p.src_d[k];
    const int nvd = (span + p.ext[k]) / V;
#pragma unroll
    for (int i = 0; i < kMultiPF; ++i) {
      const int w = min((int)threadIdx.x + i * 256, nvd - 1);
      int pos = ts + w * V;
      if (pos >= N) pos %= N;  // periodic wrap of the right reach
      if (sd)
        dreg[i] = __builtin_nontemporal_load(reinterpret_cast<const vec*>(sd + b * (size_t)N + pos));
      else
#pragma unroll
        for (int e = 0; e < V; ++e) dreg[i][e] = T(0);
    }
  };
  auto d_store = [&](int k) {
    const int2 pd = layout(k);
    const T* th = p.thr[k];
    const T thb = th ? th[b] : T(0);
    const int nvd = (span + p.ext[k]) / V;
#pragma unroll
    for (int i = 0; i < kMultiPF; ++i) {
      const int w = (int)threadIdx.x + i * 256;
      if (w < nvd) {
        vec v = dreg[i];
        if (th)
#pragma unroll
          for (int e = 0; e < V; ++e) v[e] = threshold_t(v[e], thb, p.soft);
        *reinterpret_cast<vec*>(D + phys(w, pd) * V) = v;
      }
    }
  };
  if (p.pad) {
    // a_top through registers into level top's layout (the d_load path, no threshold)
    const int2 pd = layout(top);
    const int nva = (span + p.ext[top]) / V;
#pragma unroll
    for (int i = 0; i < kMultiPF; ++i) {
      const int w = min((int)threadIdx.x + i * 256, nva - 1);
      int pos = ts + w * V;
      if (pos >= N) pos %= N;
      if (p.src_a)
        dreg[i] = __builtin_nontemporal_load(reinterpret_cast<const vec*>(p.src_a + b * (size_t)N + pos));
      else
#pragma unroll
        for (int e = 0; e < V; ++e) dreg[i][e] = T(0);
    }
#pragma unroll
    for (int i = 0; i < kMultiPF; ++i) {
      const int w = (int)threadIdx.x + i * 256;
      if (w < nva) *reinterpret_cast<vec*>(A + phys(w, pd) * V) = dreg[i];
    }
  } else {
    tile_to_lds(A, p.src_a ? p.src_a + b * (size_t)N : p.src_a, N, ts, 0, span + p.ext[top], kHaloPeriodic, 0,
                (const T*)nullptr, 0, (const T*)nullptr, T(0), 0, p.src_a == nullptr, vec_ok);
  }
  if (pf) {
    d_load(top);
    d_store(top);
  }
  for (int k = top; k >= 0; --k) {
    if (!pf) {
      const T* sd = p.src_d[k];
      const T* th = p.thr[k];
      tile_to_lds(D, sd ? sd + b * (size_t)N : sd, N, ts, 0, span + p.ext[k], kHaloPeriodic, 0, (const T*)nullptr, 0,
                  th, th ? th[b] : T(0), p.soft, sd == nullptr, vec_ok);
    }
    lds_barrier();  // A and D complete
    if (pf && k > 0) d_load(k - 1);
    const int s = p.s0 << k;
    const int nv = (span + (k > 0 ? p.ext[k - 1] : 0)) / V;  // the tile + what the next levels read
    T acc[NI][V];
    if constexpr (L > 0) {
      // Register-blocked taps (S a multiple of V): one thread owns the NI outputs v, v+m, .., v+(NI-1)m
      // (m = S/V vectors), which read the same LDS vectors shifted by one tap: NI+L-1 reads per branch
      // instead of NI*L.  Per output the taps still run i ascending, A then D: bit-identical sums.
      const int m = s / V;
      const int pairs = (nv + m * NI - 1) / (m * NI) * m;  // (block, column) pairs, uniform
      if (p.rblk && s >= V && s % V == 0 && pairs <= 256) {
        const int pr = threadIdx.x;
        const int vb = (pr / m) * m * NI + pr % m;
        const int lim = (span + p.ext[k]) / V - 1;  // last vector of the A/D regions
        const int2 pdk = layout(k), pdn = k > 0 ? layout(k - 1) : make_int2(30, 0);
#pragma unroll
        for (int r = 0; r < NI; ++r)
#pragma unroll
          for (int e = 0; e < V; ++e) acc[r][e] = T(0);
        if (pr < pairs) {
          // compile-time stride M and its layout (BlkC, vw_blk.h): the reads of a lane sit at fixed offsets off(j)
          // from phys(vb) -- with G = 8 or 4 (NI = 4, M <= 4) vectors per pad group, (vb % G) + (M*j % G) < G
          // for every M <= 8 here (vb % G = pr % M < M, or M*j % G = 0), so (vb + M*j) / G = vb / G + M*j / G --
          // and each is one ds_read at an immediate offset.
          // Reads past the region end (at most 15*M vectors, only for outputs that are never stored) stay
          // inside the allocation: the host adds p.slack >= 16*8 + 16 vectors after D (M <= 8 here).
          const T* const tlo = p.lo;
          const T* const thi = p.hi;
          auto blk_c = [&](auto mc) __attribute__((always_inline)) {
            using C = BlkC<decltype(mc)::value, NI, 0>;  // the padded layout of stride M (p.pad)
#pragma unroll
            for (int br = 0; br < 2; ++br) {
              const unsigned ab = lds_base((br == 0 ? A : D) + phys(vb, make_int2(C::SH, C::PAD)) * V);
#pragma unroll
              for (int j = 0; j < NI + L - 1; ++j) {
                const vec x = lds_vec_at<vec>(ab + (unsigned)(C::off(j) * V * (int)sizeof(T)));
#pragma unroll
                for (int r = 0; r < NI; ++r) {
                  const int i = j - r;
                  if (i >= 0 && i < L) {
                    // the tap straight from the kernel arguments (a pointer to p.lo / p.hi would copy
                    // the argument block to scratch)
                    const T fi = br == 0 ? tlo[i] : thi[i];
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[r][e] = madd<FMA>(acc[r][e], x[e], fi);
                  }
                }
                if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // bounded reads in flight (VGPRs)
              }
            }
          };
          using I1 = std::integral_constant<int, 1>;
          using I2 = std::integral_constant<int, 2>;
          using I4 = std::integral_constant<int, 4>;
          using I8 = std::integral_constant<int, 8>;
          // padded layouts only (the default, p.pad): more instantiations in this function raised it from 160
          // VGPRs to 238 + 1.3 KiB of scratch (the taps, hoisted across the switch)
          const int sel = p.slack && padded(pdk) ? m : -1;
          switch (sel) {
            case 1: blk_c(I1{}); break;
            case 2: blk_c(I2{}); break;
            case 4: blk_c(I4{}); break;
            case 8: blk_c(I8{}); break;
            default:  // (its own copy of blk_c's loop: one loop given a reader and a tap accessor compiled to other code)
#pragma unroll
              for (int br = 0; br < 2; ++br) {
                const T* buf = br == 0 ? A : D;
                const T* f = br == 0 ? p.lo : p.hi;
#pragma unroll
                for (int j = 0; j < NI + L - 1; ++j) {
                  const vec x = *reinterpret_cast<const vec*>(buf + phys(min(vb + m * j, lim), pdk) * V);
#pragma unroll
                  for (int r = 0; r < NI; ++r) {
                    const int i = j - r;
                    if (i >= 0 && i < L)
#pragma unroll
                      for (int e = 0; e < V; ++e) acc[r][e] = madd<FMA>(acc[r][e], x[e], f[i]);
                  }
                }
              }
              break;
          }
          if (k == 0) {
#pragma unroll
            for (int r = 0; r < NI; ++r)
              if (vb + m * r < nv) {
                store_vec(p.out_a + b * (size_t)N + ts, (vb + m * r) * V, cnt, vec_ok, acc[r]);
                if (p.nf_flag)
#pragma unroll
                  for (int e = 0; e < V; ++e)
                    if ((vb + m * r) * V + e < cnt) nf = nf_step<T>(acc[r][e], nf);
              }
          }
        }
        if (k == 0) break;
        lds_barrier();  // every read of A and D done
        if (pr < pairs) {
#pragma unroll
          for (int r = 0; r < NI; ++r) {
            if (vb + m * r < nv) {
              vec o;
#pragma unroll
              for (int e = 0; e < V; ++e) o[e] = acc[r][e];
              *reinterpret_cast<vec*>(A + phys(vb + m * r, pdn) * V) = o;
            }
          }
        }
        if (pf) d_store(k - 1);
        continue;
      }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int w = threadIdx.x + i * 256;
#pragma unroll
      for (int e = 0; e < V; ++e) acc[i][e] = T(0);
      if (w < nv) {
        // K4: all approximation taps, then all detail taps, into one accumulator
        inv_branch<T, L, FMA>(A, w * V, s, 1, 0, p.lo, p.taps, acc[i]);
        inv_branch<T, L, FMA>(D, w * V, s, 1, 0, p.hi, p.taps, acc[i]);
        if (k == 0) {
          store_vec(p.out_a + b * (size_t)N + ts, w * V, cnt, vec_ok, acc[i]);
          if (p.nf_flag)
#pragma unroll
            for (int e = 0; e < V; ++e)
              if (w * V + e < cnt) nf = nf_step<T>(acc[i][e], nf);
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // one vector's LDS reads in flight at a time (VGPR budget)
    }
    if (k == 0) break;
    lds_barrier();  // every read of A and D done
    const int2 pdn = layout(k - 1);  // (this level itself is never padded: see layout())
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int w = threadIdx.x + i * 256;
      if (w < nv) {
        vec o;
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = acc[i][e];
        *reinterpret_cast<vec*>(A + phys(w, pdn) * V) = o;
      }
    }
    if (pf) d_store(k - 1);
  }
  if (p.nf_flag) nf_flag_row<T>(p.nf_flag, b, nf);  // VW_FLAG_REF_NONFINITE: y's probe (vw_ref.hip)
}
}  // namespace vw
