// vw_internal.h -- what the HIP kernels (vw_dev_*.h, *.hip), the planner (vw_plan.cpp) and the C-ABI host layer
// (vw_host.h: vw_ctx.cpp, vw_exec.cpp, vw_api_*.cpp) share: constants, the kernels' argument structs and the layout
// rules both sides apply.  Plain C++: no HIP header, no launcher (those are declared in vw_launch.h).  Not installed;
// the public boundary is include/vectorwave_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include "vw_taps.h"

namespace vw {

constexpr int kMaxTaps = 64;    // longest base filter accepted (COIF10 = 60 taps)
constexpr int kMaxLevels = 24;  // batch semantics have no level cap; LDS / N bound it in practice
constexpr int kNV = 8;          // max vectors (16 B each) held per thread in the fused kernels (NV = 4 or 8)
constexpr int kMaxThreads = 1024;
constexpr int kLdsBytes = 160 * 1024;
constexpr int kSweepMinS = 16;    // per-level path: spacings >= this run as column sweeps (vw_dev_lvl.h)
constexpr int kSweepChunk = 128;  // q-chunk per sweep thread (measured: 128 beats 256 and 64)

// Source of the values outside [0, N) of a level's input ("halo"), i.e. the reference's index map.
enum HaloMode : int {
  kHaloPeriodic = 0,   // ((i % N) + N) % N        ScalarOps.java:700-723, (t+l)%N in the inverses
  kHaloZero = 1,       // 0                        ScalarOps.java:790-808, :590-601
  kHaloSymmetric = 2,  // MathUtils.symmetricBoundaryExtension  core/util/MathUtils.java:30-51
  kHaloFftPad = 3,     // i + nextPow2(N) if < N else 0 (FFT branch zero-pads)  ScalarOps.java:650-675
  kHaloHistory = 4     // streaming left history   BatchSIMDMODWT.java:447-507
};

// Per-level description, computed on the host (vw_plan.cpp forward_levels / inverse_levels) from the reference's bookkeeping.
struct LevelDesc {
  int s;        // a-trous spacing 2^(j-1)
  int hl, hr;   // halo extents (elements) the level reads left of 0 / right of N-1
  int mode;     // HaloMode of the level input (forward) / of both inverse inputs
  int dir_a;    // inverse approx branch: +1 reads t + i*s + off_a, -1 reads t - i*s + off_a
  int off_a;
  int dir_d;    // inverse detail branch
  int off_d;
  int use_d;    // inverse: 1 = d_j from memory, 0 = zero details (reconstructFromLevel / Levels)
  int hist_len; // streaming: left history length of this level (L_j - 1)
  int own;      // 1: halo written by the element owners (vw_dev_core.h halo_images), else filled after a barrier
  int il_a, il_b;  // left image of element t: il_a*t + il_b (kept when in [-hl, 0))
  int ir_a, ir_b;  // right image: ir_a*t + ir_b (kept when in [N, N+hr))
  int vs, ve;   // only vectors w < vs or w >= ve have images
};

template <typename T>
struct FwdArgs {
  const T* x;           // [B][ldx]
  long long ldx;
  T* details;           // [J][B][N]
  T* approx;            // [B][N]
  long long B;
  int N;
  int J;
  int npow2;            // nextPow2(N) for kHaloFftPad
  int hlpad;            // LDS offset of element 0 (multiple of the vector width)
  int region1;          // element offset of the second level buffer (0 = single buffer)
  int vec_io;
  int unrolled;         // 1: the tap-unrolled kernel may run (aligned rows, full slabs; vw_plan.cpp fused_plan)
  int dma_nt;           // k_forward_persist: non-temporal LDS-DMA of the signal rows
  int level_ct;         // 1: strided levels of short filters dispatch to compile-time-stride bodies, and
                        // k_forward_persist runs its full-slab form (VW_LEVEL_CT; vw_dev_rows.h fwd_row_ct)
  int validate;         // 1: non-finite check on input and outputs (atomicMin into *bad)
  int rev;              // 1: workgroup g owns signal B-1-g (walk order: VW_FWD_REV, vw_plan.h Tuning)
  unsigned long long* bad;
  // streaming history (kHaloHistory): hist[j] is [B][hist_len_j], oldest first
  T* hist[kMaxLevels];
  int hist_update;      // 1: write the new history after each level
  int taps;             // L (runtime copy; kernels are also templated on it)
  int taps_hi;          // taps of hi: == taps, except on the two-length route (VW_BI; k_forward_fused reads each tap
                        // position once and feeds the low sum while i < taps, the high sum while i < taps_hi)
  int tap_lds;          // k_forward_blk: element offset of the LDS tap table
  int blk_tight;        // k_forward_blk: sparse padding (blk_pad)
  int* nf_flag;         // k_forward_persist, VW_FLAG_REF_NONFINITE: nf_flag[b] = 1 when an output of row b is
                        // non-finite (nullptr = off; the rows vw_ref.hip recomputes)
  T lo[kMaxTaps];       // base taps * 1/sqrt(2)  (ScalarOps.java:909-916: same at every level)
  T hi[kMaxTaps];
  LevelDesc lv[kMaxLevels];
};

template <typename T>
struct InvArgs {
  const T* details;     // [J][B][N]
  const T* approx;      // [B][N]
  T* y;                 // [B][N]
  long long B;
  int N;
  int J;
  int hlpad_a, hlpad_d; // LDS offsets of element 0 in the A and D regions
  int region_d;         // element offset of the D region start in LDS
  int vec_io;
  int pair;             // 1: sum += (h*a + g*d) per tap (MODWTTransform.inverse, ZERO multi-level)
  int unrolled;
  int level_ct;         // 1: compile-time-stride level bodies (VW_LEVEL_CT; vw_dev_rows.h inv_row_ct)
  int full;             // 1: aligned rows, threads * NV == N / V: k_inverse_seq's full-slab form may run
  int plain;            // 1 (with full, fp64): PERIODIC from every coefficient plane -- all levels read t + i*s with
                        // hr <= N, no threshold, no zeroed plane, no probe, forward walk: k_inverse_seq's PLAIN form
  int waves;            // waves per SIMD of the PLAIN form's instantiation, 6 or 8 (VW_INV_WAVES)
  int db;               // sequential sum: 1 = two LDS buffers (k_inverse_db), 0 = one (k_inverse_seq)
  int blk;              // 1: register-blocked PERIODIC inverse (k_inverse_blk), padded LDS layouts
  int approx_zero;
  int rev;              // 1: workgroup g owns signal B-1-g
  const T* thr;         // thresholds [J][thr_ld] (nullptr = no thresholding)
  long long thr_ld;     // level stride of thr (0: one threshold per signal for every level)
  int soft;
  int taps;
  int taps_hi;          // taps of hi: == taps, except on the two-length route (VW_BI; k_inverse_seq / k_inverse_db run
                        // each branch at its own count: taps = the low-pass length, taps_hi the high-pass length)
  int tap_lds;          // k_inverse_blk: element offset of the LDS tap table
  int blk_tight;        // k_inverse_blk: sparse padding (blk_pad)
  int* nf_flag;         // k_inverse_seq, VW_FLAG_REF_NONFINITE: nf_flag[b] = 1 when an input or the output of
                        // row b is non-finite (nullptr = off)
  T lo[kMaxTaps];
  T hi[kMaxTaps];
  LevelDesc lv[kMaxLevels];
};

// Forward, then inverse of the same rows in one launch (vw_pair.hip k_roundtrip; fp64, L <= 8): the forward's
// arguments as k_forward_persist takes them, and what the inverse half reads besides -- inverse_seq_plain's
// share of an InvArgs (vw_plan.cpp pair_fusable: the spacings are the forward's, the level buffer is the
// forward's region from its first element on).
constexpr int kPairMaxTaps = 8;
constexpr int kPairMaxKeep = 2;   // detail planes below d_J that k_roundtrip can keep in registers (VW_PAIR_KEEP)
constexpr int kPairAutoKeep = 2;  // the most the auto rule takes: what measured best on the headline
// Which k_roundtrip variant runs (vw_plan.cpp: host-only, no HIP call): the number of kept planes, 0 .. kPairMaxKeep.
// requested (Tuning::pair_keep) >= 0 forces that variant, clamped to kPairMaxKeep.  Auto (< 0): the largest variant
// <= kPairAutoKeep whose resident workgroups per CU (per_cu[v], from the occupancy query for the launch's threads and
// LDS) are no fewer than variant 0's -- a kept plane is 16 VGPRs, and is never bought with a resident workgroup.
int pair_keep_variant(int requested, const int (&per_cu)[kPairMaxKeep + 1]);
template <typename T>
struct PairArgs {
  FwdArgs<T> f;
  T* y;                   // [B][N]
  T ilo[kPairMaxTaps];    // reconstruction taps * 1/sqrt(2)
  T ihi[kPairMaxTaps];
  int hr[kMaxLevels];     // InvArgs::lv[j].hr / .own
  int own[kMaxLevels];
};

// Per-level tiled fallback (N too large for the fused kernels): one launch per level.
template <typename T>
struct LevelArgs {
  const T* src_a;       // forward: level input [B][lda]; inverse: approx input [B][N]
  long long lda;
  const T* src_d;       // inverse: details of this level [B][N]
  const T* src_d2;      // k_inverse_sweep2/3: details of level j-1 [B][N]
  const T* thr2;        // k_inverse_sweep2/3: thresholds of level j-1
  int use_d2;
  const T* src_d3;      // k_inverse_sweep3: details / thresholds of level j-2
  const T* thr3;
  int use_d3;
  T* out_a;             // forward: approx out [B][N]; inverse: y out [B][N]
  T* out_d;             // forward: detail out [B][N]
  const T* hist;        // kHaloHistory source [B][hist_len]
  long long B;
  int N;
  int tile;             // outputs per workgroup
  int hlpad;            // LDS offset of tile element 0 (A)
  int region_d, hlpad_d;
  int pair;
  const T* thr;
  int soft;
  int use_d;
  int vec_io;
  int validate;
  unsigned long long* bad;
  int npow2;
  int taps;
  T lo[kMaxTaps];
  T hi[kMaxTaps];
  LevelDesc lv;
};

// Multi-level tiles (PERIODIC, long signals): a group of consecutive levels of one tile in one
// launch, the intermediate approximations kept in LDS (vw_dev_lvl.h k_forward_multi / k_inverse_multi).
constexpr int kMaxGroup = 8;
constexpr int kMultiInvNI = 8;  // k_inverse_multi: output vectors per thread (256 threads)
constexpr int kMultiPF = 6;     // k_inverse_multi: prefetched detail vectors per thread (256 threads)
template <typename T>
struct MultiArgs {
  const T* src_a;            // forward: input of the group's first level [B][lda]; inverse: a_{j1} [B][N] (nullptr = 0)
  long long lda;
  const T* src_d[kMaxGroup]; // inverse: d_j of group level k (k = 0 is the finest), nullptr = zero
  T* out_d[kMaxGroup];       // forward: d_j of group level k
  T* out_a;                  // forward: approximation of the coarsest level; inverse: a_{j0-1}
  const T* thr[kMaxGroup];   // inverse denoise: thresholds [B] of group level k (nullptr = none)
  long long B;
  int N;
  int tile;                  // stored outputs per workgroup (multiple of V)
  int nlev;                  // levels in the group
  int s0;                    // spacing of the group's finest level
  int ext[kMaxGroup + 1];    // forward: left extent of level k's input (ext[nlev] = 0);
                             // inverse: right extent of level k's input;
                             // multiples of V, each covering the reach of the levels after it
  int region;                // element stride between LDS buffers
  int vec_io;
  int soft;
  int taps;
  int rblk;                  // inverse: register-blocked taps where S is a multiple of V
  int pf;                    // inverse: next level's detail tile prefetched into registers
  int pad;                   // inverse: padded LDS layout at the register-blocked levels (needs pf, rblk)
  int* nf_flag;              // inverse, VW_FLAG_REF_NONFINITE, the group writes y: y's probe (nullptr = off)
  int slack;                 // inverse: LDS vectors allocated past D (compile-time-stride reads, 0 = off)
  int ni;                    // inverse: output vectors per thread, kMultiInvNI or 4 (fp64)
  T lo[kMaxTaps];
  T hi[kMaxTaps];
};

// WaveletDenoiser threshold methods (core/denoising/WaveletDenoiser.java:588-622) and the per-launch
// constants of the threshold kernels (vw_sigma.h).
enum ThrMethod { kThrUniversal = 0, kThrSure = 1, kThrMinimax = 2, kThrBayes = 3, kThrFixed = 4 };
constexpr int kSigmaRegN = 16384;  // k_noise_sigma keeps a row's keys in registers up to this N (1024 x 16)
constexpr int kSureMaxN = 16384;  // SURE on device: the sorted row lives in LDS
struct DenoiseConsts {
  double level_scale[kMaxLevels];  // Math.sqrt(1 << level) (denoiseMultiLevel, :225), 1 for denoise()
  double univ_c;                   // Math.sqrt(2.0 * Math.log(n))
  double log_n;                    // Math.log(n)
  int method;
  int n;
};

// The reference's own arithmetic for rows holding non-finite values (vw_ref.hip, VW_FLAG_REF_NONFINITE).
constexpr int kRefPlanes = 2 * kMaxLevels + 3;  // x, J details, approx, J streaming histories
template <typename T>
struct RefScan {                // flag[b] = 1 when row b of any plane is non-finite somewhere
  const T* p[kRefPlanes];
  long long ld[kRefPlanes];     // row stride of plane k
  int len[kRefPlanes];          // row length of plane k (0: N)
  int np;
  long long B;
  int N;
  int chunks;                   // ref_scan_chunks(N)
  int* flag;                    // [B], kept zero between calls (k_ref_* clear the rows they recompute)
};
template <typename T>
struct RefArgs {
  const T* x;                   // forward: input [B][ldx]; inverse: approximation [B][N] (nullptr = zeros)
  long long ldx;
  const T* det_in;              // inverse: details [J][B][N]
  T* details;                   // forward outputs [J][B][N], [B][N]
  T* approx;
  T* y;                         // inverse output [B][N]
  const T* thr;                 // inverse: thresholds [J][thr_ld] (nullptr = none)
  long long thr_ld;
  int soft;
  long long B;
  int N;
  int J;
  int L;                        // taps of lo (and of hi when Lhi == 0)
  int Lhi;                      // biorthogonal bank: taps of hi (0 = L); each filter stops at its own upsampled length
  int mode;                     // kHaloPeriodic / kHaloZero / kHaloSymmetric
  // forward, BatchStreamingMODWT ZERO / SYMMETRIC blocks: samples left of the block come from the level's
  // history (hist_old, [B][hist_len_j] oldest first; hist_first: the history the first block initialises,
  // zeros / the mirror of the level input); hist_new (nullptr: none, e.g. a flush) receives the updated one
  int hist_mode;
  int hist_first;
  const T* hist_old[kMaxLevels];
  T* hist_new[kMaxLevels];
  int hist_len[kMaxLevels];
  int* flag;                    // rows to recompute (cleared once recomputed)
  T* scratch;                   // [grid][2][N] running approximations
  T lo[kMaxTaps];               // base taps * 1/sqrt(2), as the fast kernels
  T hi[kMaxTaps];
  LevelDesc lv[kMaxLevels];     // inverse: use_d, K6 orientation / offsets
};
int ref_scan_chunks(int N);

// Financial analytics (vw_fin.hip): one workgroup per row, the row's level-1 coefficients in LDS.
constexpr int kFinMaxN = 16384;    // longest row (returns for analyze, N for the Sharpe calls): 8 * n bytes of LDS
constexpr int kFinMaxTaps = 30;
constexpr int kFinPerThread = 16;  // coefficients a thread holds in registers while they replace the row in LDS
struct FinArgs {
  const double* x;         // analyze: prices [B][ld], N per row; sharpe: returns [B][ld]
  long long ld;
  long long B;
  int N;
  int L;
  int tree;                // 1: tree reductions (VW_FLAG_TREE_SUMS), 0: the reference's sequential sums
  int validate;            // 1: non-finite inputs (and overflowed returns, bit 62) -> atomicMin into *bad
  int wavelet;             // sharpe: 1 = level-1 forward + inverse with zero details first (PERIODIC)
  double k;                // analyze: anomaly threshold in standard deviations; sharpe: risk-free rate
  double* out;             // analyze: [5][B]; sharpe: [B]
  unsigned long long* bad;
  double lo[kFinMaxTaps];  // base taps * 1/sqrt(2), as the transform kernels
  double hi[kFinMaxTaps];
};

// Wavelet energy per level (vw_energy.hip): out[0][b] = sum a_J[b][t]^2, out[j][b] = sum d_j[b][t]^2, fp64.
constexpr int kEnergyWaves = kMaxThreads / 64;
constexpr int kEnergyRed = (kMaxLevels + 1) * kEnergyWaves;  // LDS doubles behind the level buffers: one partial
                                                             // per (plane, wave)
constexpr int kEnergyUnrollMax = 8;  // longest filter with a tap-unrolled k_energy_fused (vw_energy.hip launch_energy_fused)
// Fused energy forward (k_energy_fused): k_forward_fused's cascade with the stores replaced by sums of squares.
struct EnergyArgs {
  const double* x;      // [B][ldx]
  long long ldx;
  double* out;          // [J+1][B]
  long long B;
  int N;
  int J;
  int npow2;
  int hlpad;            // LDS offset of element 0 (as FwdArgs)
  int region1;          // element offset of the second level buffer (0 = single buffer)
  int red_off;          // element offset of the [J+1][kEnergyWaves] wave partials
  int vec_io;
  int unrolled;
  int level_ct;
  int taps;
  double lo[kMaxTaps];  // base taps * 1/sqrt(2)
  double hi[kMaxTaps];
  LevelDesc lv[kMaxLevels];
};
// Energies of coefficient planes already in memory: approx [B][N], details [J][B][N] (nullptr when J = 0).
struct EnergyPlanesArgs {
  const double* approx;
  const double* details;
  long long B;
  int N;
  int J;
  int vec_io;           // 1: N even and both arrays 16-byte aligned (every row then is)
  double* out;          // [J+1][B]
};

// Multiresolution analysis (vw_mra.hip k_mra): out[0] = the smooth (a_J alone), out[c] = detail component c (d_c
// alone), each the masked inverse with the branch passes over zeroed planes left out.
constexpr int kMraUnrollMax = 14;  // longest filter with a tap-unrolled k_mra (vw_mra.hip launch_mra): from 16 taps on
                                   // some instantiations spill to scratch
template <typename T>
struct MraArgs {
  const T* details;     // [J][B][N]
  const T* approx;      // [B][N]
  T* out;               // [J+1][B][N]
  long long B;
  int N;
  int J;
  int hlpad;            // LDS offset of element 0 (multiple of the vector width)
  int region1;          // element offset of the second region (the two are used ping-pong)
  int vec_io;
  int unrolled;
  int level_ct;
  int taps;
  T lo[kMaxTaps];       // base taps * 1/sqrt(2)
  T hi[kMaxTaps];
  LevelDesc lv[kMaxLevels];  // inverse_levels' descriptors: dir_a / off_a / dir_d / off_d per branch
};

// Continuous wavelet transform (vw_cwt.hip k_cwt): out[b][s][tau] = (sum_k w_s[k] * ext(x_b, tau + o_s + k)) / q_s,
// k ascending from an accumulator at +0.0 -- CWTTransform.analyzeDirect / analyzeDirectComplex (:120-218) with the
// table w_s[k] = psi(-(k - H)/s)/sqrt(s), o_s = -H, q_s = 1, and analyzeFFT (:223-318) as the shifted sum over the
// zero-padded FFT period (kCwtWrapZero, o_s = +H, q_s = sqrt(s)).
enum CwtExt : int {        // ext(x, i) outside [0, N): CWTTransform.getBoundaryValue :354-396
  kCwtZero = 0,            // 0
  kCwtReflect = 1,         // i < 0: x[min(-i, N-1)];      i >= N: x[max(2N - i - 2, 0)]
  kCwtSymmetric = 2,       // i < 0: x[min(-i - 1, N-1)];  i >= N: x[max(2N - i - 1, 0)]
  kCwtPeriodic = 3,        // x[((i % N) + N) % N]
  kCwtWrapZero = 4         // m = i mod M: x[m] when m < N, else 0 (the FFT branch's zero-padded period M)
};
constexpr int kCwtChunkBytes = 32;  // a thread's NV adjacent outputs: 32 bytes of elements (NV = 4 fp64, 8 fp32)
constexpr int kCwtThreads = 256;    // most threads of a k_cwt workgroup (tile = threads * NV outputs)
constexpr int kCwtMaxTaps = 16384;  // longest table of one scale the planner places (Morlet at scale 2048)
constexpr int kCwtMaxGrid = 1 << 20;  // workgroups per launch; the kernel strides over the work items beyond
// Chunks of NV elements a workgroup stages for a scale of K taps, the one rule of the planner (LDS bytes =
// chunks * kCwtChunkBytes) and the kernel: thread t reads chunks t .. t + K / NV + 1.  Odd, so that the two 16-byte
// planes of the chunks (vw_cwt.hip cwt_slot) start on different halves of a 256-byte bank row.
constexpr int cwt_chunks(int threads, int K, int nv) { return (threads + K / nv + 1) | 1; }
// One scale as the kernel reads it (device memory, heaviest first), T-typed divisor.
template <typename T>
struct CwtScaleDev {
  int tap_begin;   // first tap in taps_re / taps_im
  int taps;        // K_s
  int window;      // o_s
  int scale;       // the caller's scale index (output plane)
  T divisor;       // q_s
};
template <typename T>
struct CwtArgs {
  const T* x;                  // [B][ldx]
  long long ldx;
  T* out_re;                   // [B][S][N]
  T* out_im;                   // [B][S][N], complex tables only
  const T* taps_re;            // device tables, rounded to T once on the host
  const T* taps_im;
  const CwtScaleDev<T>* sc;    // the launch's scales
  long long B;
  int N;
  int S;                       // scales of the whole call (the stride of a row's planes)
  int nsc;                     // scales of this launch
  int ntiles;                  // ceil(N / (threads * NV))
  int ext;                     // CwtExt
  long long wrap;              // M of kCwtWrapZero
};

// Inverse continuous wavelet transform (vw_icwt.hip): InverseCWT.reconstruct (cwt/InverseCWT.java) on coefficient
// planes [B][S][ldc] into rows [B][ldo].
//   kIcwtSum     out[b][tau] = (sum_j weight_j * (sum_k w_j[k] * z_{b,plane_j}[(tau + o_j + k) mod wrap])) / divisor, z zero
//                on [N, wrap): what reconstructInternalRealFFT (:225-270) evaluates by FFT.  One accumulator per
//                descriptor from +0.0, k ascending; one outer accumulator from +0.0, j ascending (k_icwt).
//   kIcwtDirect  reconstructInternalRealDirect's loops (:283-311): one accumulator over j and b ascending of
//                ((c * w_j[t - b + N - 1]) * weight_j) / scale_j, terms with |c| < 1e-10 skipped (k_icwt_direct).
enum IcwtForm : int { kIcwtSum = 0, kIcwtDirect = 1 };
constexpr int kIcwtDirectThreads = 64;  // a k_icwt_direct workgroup: one thread per output
// One descriptor as the kernels read it (device memory, the caller's order), weight and scale rounded to T once.
template <typename T>
struct IcwtScaleDev {
  int tap_begin;   // first tap in taps
  int taps;        // K_j
  int window;      // o_j
  int plane;       // the coefficient plane it reads
  T weight;
  T scale;         // kIcwtDirect only
};
template <typename T>
struct IcwtArgs {
  const T* coef;               // [B][S][ldc]
  long long ldc;
  T* out;                      // [B][ldo]
  long long ldo;
  const T* taps;               // device table, rounded to T once on the host
  const IcwtScaleDev<T>* sc;   // the call's descriptors
  long long B;
  int N;
  int S;                       // planes per row
  int nsc;                     // descriptors
  int ntiles;                  // ceil(N / (threads * NV)), kIcwtSum
  long long wrap;              // M, kIcwtSum
  T divisor;
};

// Register-blocked kernels (vw_blk.h k_forward_blk / k_inverse_blk, and k_inverse_multi's blocked levels):
// the padded LDS layout of a level with vector stride m and nv outputs per thread, the one rule for the
// planner (buffer sizes) and the kernels (addresses).  NV = 4: one pad vector per 4 (m <= 4), two per 8
// (m = 8); NV = 8: one per 8 (m <= 8); none for m >= 16 or m = 0 (s < V: the standard mapping).
// tight (the standard layout does not fit LDS, e.g. sym8 at N = 16384): NV = 8 pads one vector per 16 --
// 6 % of LDS instead of 12.5 %, 1.3-2x the conflict-free cycles, still 3-4x fewer than the
// one-vector-per-tap reads.
struct BlkLayout {
  int sh, pad;  // logical vector u -> u + (u >> sh) * pad
};
constexpr BlkLayout blk_pad(int m, int nv, int tight = 0) {
  if (m <= 0 || m >= 16) return BlkLayout{30, 0};
  if (nv >= 8) return tight ? BlkLayout{4, 1} : BlkLayout{3, 1};
  if (m == 8) return BlkLayout{3, 2};
  return BlkLayout{2, 1};
}

}  // namespace vw
