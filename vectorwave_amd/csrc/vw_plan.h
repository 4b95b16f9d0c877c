// vw_plan.h -- kernel selection of the forward and inverse transforms, as a pure host function of the
// call's shape, flags and pointer alignments, the tuning switches and the CU count.  plan_forward /
// plan_inverse make no HIP call and touch no memory behind the caller's pointers; vw_exec.cpp executes
// what they return (reserve, launch, fix up) and decides nothing itself.  Compiles with a plain C++
// compiler (tests/plan_harness checks every plan against the kernels' launch contracts on the CPU).
#pragma once
#include "../../include/vectorwave_amd.h"
#include "vw_internal.h"
#include "vw_deep.h"

#include <vector>

namespace vw {

// Tuning switches (A/B experiments, tools/ab_*.sh), read from the environment ONCE per context at
// vw_ctx_create -- never per call: a transform call does no getenv.  Defaults are the measured best.
// Names, clamping and the order of the environment scan: kTuningTable (vw_plan.cpp).
struct Tuning {
  int nv = 4;              // VW_NV: vectors per thread of the fused kernels (4 or 8)
  bool fwd_persist = true; // VW_FWD_PERSIST=0: no persistent forward
  int fwd_buf = 0;         // VW_FWD_BUF=1|2: force one / two forward level buffers (0 = policy)
  bool force_tiled = false;// VW_FORCE_TILED: per-level path even when the fused kernels fit
  int fwd_rev = 0, inv_rev = 0;  // VW_FWD_REV / VW_INV_REV: reverse workgroup -> signal walk
  int dma_nt = -1;               // VW_DMA_NT=0|1: LDS-DMA of signal rows non-temporal; -1 = policy (see plan_forward)
  int fwd_tile = 0;        // VW_FWD_TILE: per-level forward tile (0 = default)
  bool multi = true;       // VW_MULTI=0: one launch per level on the long-signal path
  int multi_div = 4;       // VW_MULTI_DIV: reach bound of a level group = tile / div
  int multi_tile = 0;      // VW_MULTI_TILE: multi-level tile (0 = 16 KiB of samples)
  int inv_buf = 0;         // VW_INV_BUF=2: two-buffer sequential inverse (k_inverse_db)
  int inv_tile = 0;        // VW_INV_TILE: per-level inverse tile (0 = 1024)
  int multi_rblk = 1;      // VW_MULTI_RBLK: register-blocked taps in k_inverse_multi
  int multi_pf = 1;        // VW_MULTI_PF: k_inverse_multi prefetches the next detail tile
  int multi_pad = 1;       // VW_MULTI_PAD: k_inverse_multi's padded LDS layout at register-blocked levels
  int multi_inv_tile = 0;  // VW_MULTI_INV_TILE: k_inverse_multi's tile (0 = VW_MULTI_TILE's)
  int multi_ni = 4;        // VW_MULTI_NI: k_inverse_multi's output vectors per thread -- 4 (fp64, on the largest tile
                           // whose levels fit 256 threads) or 8; db8-stream inverse 9.19-9.33 -> 8.75-8.80 ms
                           // (profiles/r05/ab_db8_inverse_multi_ni4.log)
  bool no_sweep = false;   // VW_NO_SWEEP: no column sweeps for deep levels
  int sweep_qc = kSweepChunk;  // VW_SWEEP_QC: q-chunk per sweep thread
  int unroll_max = kMaxTaps;   // VW_UNROLL_MAX: longest filter that runs the tap-unrolled fused kernels
  int blk = 10;                // VW_BLK: shortest filter that runs the register-blocked PERIODIC kernels (0 = off)
                               // (measured on MI355X, db8 J=10 2^20 blocks: no faster than the sweeps yet)
  bool deep = true;             // VW_DEEP=0|1: streaming deep-level forward (vw_deep.hip) off / on
  bool deep_inv = false;       // VW_DEEP_INV=1 (or VW_DEEP=1): the deep inverse too -- measured slower than
                               // the column sweeps on db8-stream (profiles/r03/ab_deep_db8_stream.log)
  int deep_lds = 80;           // VW_DEEP_LDS: LDS budget of one deep group, KiB (80 = two workgroups per CU)
  int deep_waves = 4;          // VW_DEEP_WAVES: target deep workgroups per CU when choosing segments
  int deep_pf_fwd = 1;         // VW_DEEP_PF_FWD / VW_DEEP_PF_INV: tiles of DMA-fed input in flight
  int deep_pf_inv = 1;
  int fwd_nv = 0;              // VW_FWD_NV / VW_INV_NV = 2: 1024-thread fused kernels with 2 vectors per
  int inv_nv = 0;              // thread (L <= 8, unrolled); 0 = policy
  int sweep2 = 3;              // VW_SWEEP2: deep inverse column-sweep levels chained per launch, up to 3 (2 = pairs only,
                               // 0 = one sweep per level)
  int sweep2_ka = 8;           // VW_SWEEP2_KA: stage-A outputs per thread and step (8 or 16)
  int sweep2_uc = 2048;        // VW_SWEEP2_UC: u positions per workgroup chunk (512 / 1024 / 2048: 9.68 / 9.50 / 9.33 ms db8 inverse)
  int sweep2_r = 0;            // VW_SWEEP2_R=32: 32-residue groups even where h allows 64 (0 = widest)
  int sweep2_minb = 64;        // VW_SWEEP2_MINB: blocks a residue class needs for the chained sweeps
  int blk_fwd8 = 1;            // VW_BLK_FWD8=0: fused forward instead of the register-blocked one at NV = 8
  int ref_grid = 0;            // VW_REF_GRID: workgroups of the REF_NONFINITE fix-up launch (0 = 2 per CU)
  int level_ct = 1;            // VW_LEVEL_CT=0: run-time level strides and bounds-checked slabs in the fused kernels of
                               // short filters (L <= 8), as before (profiles/r07/ab_db4_level_ct.log)
  int mfma = 0;                // VW_MFMA=1|2|3: fp32 FMA PERIODIC forward (1) / inverse (2) / both (3) on the matrix
                               // cores (vw_mfma.hip)
  int energy_fused = 1;        // VW_ENERGY_FUSED=0: vw_modwt_energy_f64 never runs the fused energy kernel (forward
                               // into the workspace, then the plane sums), also under VW_FLAG_TREE_SUMS
  int bi = 3;                  // VW_BI=0: two-length banks on the padded route only; bit 0: the fused forward
                               // (k_forward_fused), bit 1: the sequential fused inverses (k_inverse_seq / k_inverse_db)
                               // run each filter at its own tap count where they fit (1 | 2 | 3, as VW_MFMA) and
                               // the pair has compile-time kernels (VW_TAP_PAIR_LIST); bit 2: every other pair too, on
                               // the runtime-L bodies (measured 2-3 x slower than the padded route's unrolled kernels)
  int inv_waves = 6;           // VW_INV_WAVES=6|8: waves per SIMD k_inverse_seq's PLAIN form is compiled for -- 8 (64 VGPRs)
                               // lets four 512-thread workgroups share a CU where 6 lets three; measured no
                               // faster than 6 on the db4 step (profiles/r09/ab_db4_inv_waves.log)
  int mra_fused = 1;           // VW_MRA_FUSED=0: vw_mra_planes_* / vw_modwt_mra_* never run k_mra (J+1 masked inverses instead);
                               // 2: k_mra wherever it fits, also where it measured slower than the loop (plan_mra)
  int pair_fuse = 1;           // VW_PAIR_FUSE=0: a captured forward and the inverse that follows it stay two kernels;
                               // 1: one k_roundtrip launch where pair_fusable holds (vw_exec.cpp)
  int pair_keep = -1;          // VW_PAIR_KEEP=0|1|2: k_roundtrip keeps that many detail planes below d_J in registers instead
                               // of reading them back (larger values: 2); < 0: auto, see pair_keep_variant (vw_internal.h)
  int bi_listed = 1;           // VW_BI_LISTED=0: a two-length bank runs max(Llo, Lhi) taps even where that count is not in
                               // VW_TAP_LIST (the runtime-L kernels); 1: one more zero tap where that reaches a listed count
};

// One switch of the Tuning struct by its environment name; value < 0 = the default.  Returns false
// for an unknown name.
bool set_tuning(Tuning& t, const char* key, int v);
Tuning read_tuning();  // the defaults, then every switch present in the environment

// ------------------------------------------------------------------------------------------------
// Bookkeeping restated from the reference, shared with the C ABI (vw_max_levels / vw_upsampled_length).
int max_levels(int64_t N, int L);
int64_t upsampled_length(int L, int level);
int ref_mode(int boundary);  // VW_PERIODIC / VW_ZERO_PADDING / VW_SYMMETRIC -> HaloMode

// ------------------------------------------------------------------------------------------------
// What a call looks like to the planner.  Pointers are the caller's: the planner reads their low four
// bits and whether they are null, the executor reads everything.  lo / hi / soft are the executor's only.
template <typename T>
struct FwdCall {
  const T* x = nullptr;
  int64_t B = 0, N = 0, ldx = 0;
  const double* lo = nullptr;
  const double* hi = nullptr;
  int L = 0, boundary = VW_PERIODIC, J = 1;
  unsigned flags = 0;
  T* details = nullptr;
  T* approx = nullptr;
  bool single_level = false;
  int mode_override = -1;        // >= 0: every level reads its halo in this HaloMode (streaming blocks)
  T* const* hist = nullptr;      // streaming histories [J], nullptr = none
  bool hist_update = false;
  T* const* hist_snap = nullptr; // VW_FLAG_REF_NONFINITE: where the histories this block reads are kept
  bool hist_first = false;
  int cus = 256;                 // compute units of the device
  int Lhi = 0;                   // biorthogonal bank: taps of `hi` when they differ from L, those of `lo` (0 = L)
};

template <typename T>
struct InvCall {
  const T* details = nullptr;
  const T* approx = nullptr;
  int64_t B = 0, N = 0;
  const double* lo = nullptr;
  const double* hi = nullptr;
  int L = 0, wid = VW_WID_OTHER, boundary = VW_PERIODIC, J = 1;
  unsigned detail_mask = ~0u;
  int approx_zero = 0;
  unsigned flags = 0;
  T* y = nullptr;
  bool single_level = false;
  const T* thr = nullptr;        // thresholds [J][thr_ld] (nullptr = none)
  int soft = 0;
  int64_t thr_ld = 0;
  int cus = 256;
  int Lhi = 0;                   // biorthogonal bank: taps of `hi` when they differ from L, those of `lo` (0 = L)
};

// ------------------------------------------------------------------------------------------------
// The plan.  Fused path (`fused`): one launch of `kernel` with `threads` x `nv` vectors and `lds` bytes;
// `args` holds every non-pointer field of the kernel's argument struct (level descriptors with their halo
// images included).  Per-level path: `steps` in launch order, each reading buffer `src` and writing `dst`.
enum PlanKernel : int {
  kFwdFused, kFwdPersist, kFwdBlk, kFwdMfma,             // forward, fused path
  kInvPair, kInvSeq, kInvDb, kInvBlk, kInvMfma,          // inverse, fused path (launch_inverse_fused picks the
                                                         // first four from args.pair / db / blk, as named here)
  kStepDeep, kStepMulti, kStepSweepG, kStepSweep, kStepTile  // per-level path
};
enum PlanBuf : int { kBufNone, kBufIn, kBufWs0, kBufWs1, kBufOut };  // caller input (x / approx), workspace halves,
                                                                     // caller output (approx / y)

template <typename T>
struct PlanStep {
  int kind;            // kStepDeep .. kStepTile
  int jlo, jhi;        // levels the launch covers
  int src, dst;        // PlanBuf
  int lds;             // dynamic LDS bytes (0: the sweeps' static rings)
  int G, ka, R;        // kStepSweepG: launch_inverse_sweepg's levels (2 / 4), outputs per thread, residues
  int probe;           // the launch writes a_J / y and probes it (VW_FLAG_REF_NONFINITE)
  int hist_update;     // forward tile: the level's history is rewritten after it
  union {              // non-pointer fields filled; the one `kind` names
    LevelArgs<T> lvl;  // kStepSweepG, kStepSweep, kStepTile
    MultiArgs<T> multi;
    DeepArgs<T> deep;
  };
};

struct PlanReserve {
  size_t ws_bytes = 0;   // workspace: the per-level path's two planes, the fix-up's scratch rows
  int64_t nf_rows = 0;   // row flags: a probing kernel or the fix-up's scan
  int ref_grid = 0;      // workgroups of the fix-up launch (0 = no fix-up)
};

template <typename T, typename Args>
struct Plan {
  int error = VW_OK;     // != VW_OK: the call cannot run; `msg` says why
  char msg[96] = "";
  bool fused = false;
  int kernel = kFwdFused;
  int threads = 0, nv = 4, lds = 0;
  bool fma = false, validate = false;
  bool snapshot = false; // forward: copy the histories the block reads before the first launch
  bool ref_nf = false;   // the reference fix-up runs after the launches
  bool nf_probed = false;// the last writer flagged the rows itself (no scan pass)
  PlanReserve res;
  Args args{};           // fused: the launch's arguments; both paths: args.lv[0 .. J) are the level descriptors
  std::vector<PlanStep<T>> steps;
};
template <typename T> using FwdPlan = Plan<T, FwdArgs<T>>;
template <typename T> using InvPlan = Plan<T, InvArgs<T>>;

// vw_modwt_energy_f64 (vw_energy.hip): whether the fused energy kernel runs and with what launch shape.  Not
// fused: the executor runs plan_forward's plan into its workspace and sums the planes there.
struct EnergyPlan {
  bool fused = false;
  bool fma = false;
  int threads = 0, nv = 4, lds = 0;
  int grid = 0;          // workgroups (grid-stride over the rows)
  EnergyArgs args{};     // every non-pointer field
};
void plan_energy(const Tuning& tu, const FwdCall<double>& c, EnergyPlan* p);

// vw_mra_planes_* / vw_modwt_mra_* (vw_mra.hip): whether k_mra runs and with what launch shape.  `c` is the inverse's
// call with y = out [J+1][B][N]; its detail_mask / approx_zero are not read.  Fused where two LDS regions (the row
// plus the longest level's halos for both branches) fit with fused_plan's thread and NV choice; never for
// single_level, VW_FORCE_TILED, VW_FLAG_VALIDATE / VW_FLAG_REF_NONFINITE (k_mra skips the zeroed planes, which
// only finite data allows), a two-length bank or VW_MRA_FUSED=0.  Not fused: the LOOP PATH -- the executor issues
// J+1 masked inverses (plan_inverse each), component c into out[c]: the same bits on any shape the inverse takes.
template <typename T>
struct MraPlan {
  bool fused = false;
  bool fma = false;
  int threads = 0, nv = 4, lds = 0;
  int grid = 0;          // workgroups (grid-stride over the rows)
  MraArgs<T> args{};     // every non-pointer field
};
template <typename T> void plan_mra(const Tuning& tu, const InvCall<T>& c, MraPlan<T>* p);

// vw_cwt_* (vw_cwt.hip k_cwt): the launch shape of a continuous wavelet transform.  One thread count for the call
// -- whole waves covering the row in chunks of NV = 32 bytes / element size outputs, at most kCwtThreads -- hence one
// tile length (threads * NV) and tile count.  Per scale: the staged chunks (cwt_chunks) and their LDS bytes.  The
// scales run heaviest first (K descending, ties in the caller's order), in launches of neighbours whose LDS need
// falls in the same power-of-two class from 16 KiB up, so a light scale keeps the occupancy a heavy one cannot have;
// a launch's LDS is its first (heaviest) scale's.  A scale with K > kCwtMaxTaps is refused: error
// VW_ERR_UNSUPPORTED, `msg` names it, nothing else of the plan is valid.
struct CwtCall {
  int64_t B = 0, N = 0;
  int S = 0;
  const int* taps = nullptr;  // K_s per scale (>= 1, checked by the caller)
  int elem_bytes = 8;
  bool cplx = false;
  int ext = kCwtZero;
  unsigned flags = 0;
};
struct CwtScalePlan {
  int scale;            // the caller's index
  int taps;
  int tile, nv, threads;
  int chunks, lds;      // staged chunks of nv elements; lds = chunks * kCwtChunkBytes
};
struct CwtLaunch {
  int first, count;     // scales order[first .. first + count)
  int lds;
  int grid;             // workgroups: min(count * ntiles * B, kCwtMaxGrid)
};
struct CwtPlan {
  int error = VW_OK;
  char msg[96] = "";
  bool fma = false, cplx = false;
  int threads = 0, nv = 0, tile = 0, ntiles = 0;
  std::vector<CwtScalePlan> order;   // heaviest first
  std::vector<CwtLaunch> launches;
};
void plan_cwt(const CwtCall& c, CwtPlan* p);

// vw_icwt_* in the SUM form (vw_icwt.hip k_icwt): one workgroup per (row, time tile) loops over every descriptor, so
// the call has one launch.  Threads, NV and the tile as plan_cwt; the staged chunks and the LDS are those of the
// call's longest table (cwt_chunks), every shorter one stages into the same bytes.  grid = min(B * ntiles,
// kCwtMaxGrid), the kernel strides over the rest.  A descriptor with K > kCwtMaxTaps is refused: error
// VW_ERR_UNSUPPORTED, `msg` names it, nothing else of the plan is valid.
struct IcwtCall {
  int64_t B = 0, N = 0;
  int nsc = 0;
  const int* taps = nullptr;  // K_j per descriptor (>= 1, checked by the caller)
  int elem_bytes = 8;
  unsigned flags = 0;
};
struct IcwtPlan {
  int error = VW_OK;
  char msg[96] = "";
  bool fma = false;
  int threads = 0, nv = 0, tile = 0, ntiles = 0;
  int max_taps = 0;     // the longest table
  int chunks = 0, lds = 0;
  int grid = 0;
};
void plan_icwt(const IcwtCall& c, IcwtPlan* p);

// Banks with two lengths (Lhi != 0 and != L; the _bi_ entry points) run the same kernels on the PADDED ROUTE: the
// shorter filter is zero-extended to args.taps = max(L, Lhi), or one tap further where only that count has
// tap-unrolled kernels (VW_BI_LISTED, vw_plan.cpp listed_taps) -- for finite data a trailing 0 * x adds +-0 to a
// sum that started at +0.0, the same bits -- while the bookkeeping keeps the true lengths: the FFT-switch mode
// per filter (a level where exactly one filter takes the reference's FFT branch is VW_ERR_UNSUPPORTED), the
// SYMMETRIC shifts tau(L) / tau(Lhi) per branch, halos over the longer reach.  The pairwise inverses (single
// level, ZERO_PADDING) loop over l < L and read hi[l]: args.taps = L with hi truncated when Lhi >= L,
// VW_ERR_UNSUPPORTED when Lhi < L (the reference indexes past its high-pass array).  The executor copies the
// taps accordingly (vw_host.h copy_bank).
// TWO-LENGTH ROUTE (VW_BI): where the non-persistent fused forward (k_forward_fused, no history) or the fused
// sequential-sum inverse (k_inverse_seq / k_inverse_db) fits at NV = 4 / 8, args.taps = L and args.taps_hi = Lhi.  The
// forward reads each tap position once and feeds the low sum while i < L, the high sum while i < Lhi; each inverse
// branch issues its own filter's LDS reads (bior3.9's synthesis 4 + 20 against the padded route's 20 + 20).  Halos are
// still sized for the longer reach.  The persistent, register-blocked and matrix-core kernels, the per-level path and
// the pairwise sums stay on the padded route.
// `p` must be a freshly constructed plan.
template <typename T> void plan_forward(const Tuning& tu, const FwdCall<T>& c, FwdPlan<T>* p);
template <typename T> void plan_inverse(const Tuning& tu, const InvCall<T>& c, InvPlan<T>* p);

// Whether a forward call and the inverse call that follows it are one round trip that k_roundtrip (vw_pair.hip) computes
// with the bits of the two kernels their plans name.  Pure: reads the calls and their plans, nothing behind a
// pointer.  True only when
//   - the forward plans to kFwdPersist in its full-slab form (fp64, NV = 4, a listed tap count <= kPairMaxTaps);
//   - the inverse plans to the PLAIN class (InvArgs::plain), or to the two-buffer kernel small batches get
//     (kInvDb) on a call that meets every condition of that class: the same sums in the same order;
//   - both calls have the same B, N, J, tap count, PERIODIC boundary and accumulation mode, one filter length each;
//   - the forward's details / approx (dense [J][B][N] and [B][N]) are the inverse's inputs;
//   - the inverse keeps every level and the approximation, without a threshold;
//   - neither call has VW_FLAG_VALIDATE, VW_FLAG_REF_NONFINITE or VW_FLAG_HOST_MEMORY;
//   - y overlaps none of x, details, approx;
//   - the inverse's right halos fit the forward's level regions (the kernel works in those).
// Each call's own plan is what it was: the plan text (describe()) does not change.
template <typename T>
bool pair_fusable(const FwdCall<T>& fc, const FwdPlan<T>& fp, const InvCall<T>& ic, const InvPlan<T>& ip);

}  // namespace vw
