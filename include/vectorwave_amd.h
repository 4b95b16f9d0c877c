/*
 * vectorwave_amd.h -- C ABI of the MI355X (gfx950) MODWT / SWT engine.
 *
 * Drop-in boundary for VectorWave's MODWT/SWT hot path: the per-level a-trous
 * low/high-pass convolutions (forward and inverse, PERIODIC / ZERO_PADDING /
 * SYMMETRIC).  Plain C types only -- no torch, no HIP types in signatures --
 * so a JNI (or Java 22+ FFM) shim, ctypes, or C/C++ host code can bind it.
 *
 * Reference interfaces each entry point replaces (paths relative to
 * /root/reference, prefixes core/ = vectorwave-core/src/main/java/com/morphiqlabs/wavelet/,
 * ext/ = vectorwave-extensions/src/main/java/com/morphiqlabs/wavelet/):
 *
 *   vw_modwt_forward_*      MultiLevelMODWTTransform.decompose / decomposeMutable
 *                             core/modwt/MultiLevelMODWTTransform.java:209-330
 *                           BatchMODWT.multiLevelAoS  ext/extensions/modwt/BatchMODWT.java:90-111
 *                           BatchSIMDMODWT.batchMultiLevelMODWTSoA  ext/extensions/modwt/BatchSIMDMODWT.java:343-424
 *                           VectorWaveSwtAdapter.forward  core/swt/VectorWaveSwtAdapter.java:198-394
 *   vw_modwt_inverse_*      MultiLevelMODWTTransform.reconstruct / reconstructFromLevel / reconstructLevels
 *                             core/modwt/MultiLevelMODWTTransform.java:339-446, :554-645
 *                           BatchMODWT.inverseMultiLevelAoS  ext/extensions/modwt/BatchMODWT.java:151-178
 *                           VectorWaveSwtAdapter.inverse / extractLevel  core/swt/VectorWaveSwtAdapter.java:435-487, :576-598
 *   vw_modwt1_forward_*     MODWTTransform.forward / forwardBatch  core/modwt/MODWTTransform.java:131-189, :486-614
 *                           BatchMODWT.singleLevelAoS  ext/extensions/modwt/BatchMODWT.java:62-79
 *   vw_modwt1_inverse_*     MODWTTransform.inverse / inverseBatch  core/modwt/MODWTTransform.java:203-299, :531-689
 *                           BatchMODWT.inverseSingleLevelAoS  ext/extensions/modwt/BatchMODWT.java:122-139
 *   vw_swt_denoise_*        VectorWaveSwtAdapter.denoise  core/swt/VectorWaveSwtAdapter.java:532-562
 *   vw_noise_sigma_*        VectorWaveSwtAdapter.estimateNoiseSigma  core/swt/VectorWaveSwtAdapter.java:627-645
 *   vw_threshold_*          MutableMultiLevelMODWTResult.applyThreshold  core/modwt/MutableMultiLevelMODWTResult.java:83-114
 *   vw_wavelet_denoise_*    WaveletDenoiser.denoise / denoiseMultiLevel / denoiseFixed
 *                             core/denoising/WaveletDenoiser.java:111-549
 *   vw_transpose_*          BatchSIMDMODWT.convertToSoA / convertFromSoA  ext/extensions/modwt/BatchSIMDMODWT.java:282-308
 *   vw_stream_*             BatchStreamingMODWT  ext/extensions/modwt/BatchStreamingMODWT.java:55-275
 *   vw_fin_analyze_*        FinancialAnalyzer.analyzeCrashAsymmetry / analyzeVolatility / analyzeRegimeTrend /
 *                             detectAnomalies  fin/FinancialAnalyzer.java:52-198
 *                             (fin/ = vectorwave-core/src/main/java/com/morphiqlabs/financial/)
 *   vw_fin_sharpe_*         FinancialWaveletAnalyzer.calculateSharpeRatio  fin/FinancialWaveletAnalyzer.java:95-124
 *   vw_fin_wavelet_sharpe_* FinancialWaveletAnalyzer.calculateWaveletSharpeRatio  fin/FinancialWaveletAnalyzer.java:166-212
 *   vw_modwt_energy_f64 /   MultiLevelMODWTResult.getDetailEnergyAtLevel / getApproximationEnergy / getTotalEnergy /
 *   vw_energy_planes_f64      getRelativeEnergyDistribution  core/modwt/MultiLevelMODWTResultImpl.java:91-139, :211-216
 *   vw_mra_planes_* /       VectorWaveSwtAdapter.extractLevel for every level  core/swt/VectorWaveSwtAdapter.java:576-598
 *   vw_modwt_mra_*            MultiLevelMODWTTransform.reconstructLevels  core/modwt/MultiLevelMODWTTransform.java:398-446
 *   vw_max_levels           MultiLevelMODWTTransform.getMaximumLevels  core/modwt/MultiLevelMODWTTransform.java:455-501, :693-695
 *   status codes            core/exception/ErrorCode.java:24-118 (see the table below)
 *
 * Memory: by default every array argument is a DEVICE pointer (hipMalloc /
 * torch CUDA storage) on the context's device, and work is enqueued on the
 * context's stream (the call returns after enqueueing unless VW_FLAG_SYNC or
 * validation needs a result).  With VW_FLAG_HOST_MEMORY all arrays are host
 * pointers: the engine stages them through its own device workspace and the
 * call is synchronous (the JNI/FFM path).  Filter taps (lo/hi) are always host
 * pointers of L doubles: the caller passes wavelet.lowPassDecomposition() /
 * highPassDecomposition() (== reconstruction filters for orthogonal
 * wavelets), exactly as the reference reads them.
 *
 * Layout: x[B][ldx] row-major (row b at x + b*ldx, ldx >= N), details
 * [J][B][N] (level 1 = finest first; BatchMODWT's detailPerLevel order),
 * approx [B][N], y [B][N].
 *
 * Threading: a context may be used from several host threads (calls are
 * serialized by its mutex and run on its stream); several contexts -- on one
 * device or on several -- run concurrently from different threads, e.g. through
 * vw_modwt_forward_multi_f64.  The engine retains no caller buffer after a
 * call returns (host-memory calls stage through a pool the context keeps).
 */
#ifndef VECTORWAVE_AMD_H
#define VECTORWAVE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VW_API __attribute__((visibility("default")))

typedef struct vw_ctx vw_ctx;
typedef struct vw_stream vw_stream;
typedef int vw_status;

/* Status codes.  Reference ErrorCode (core/exception/ErrorCode.java) -> status. */
enum {
    VW_OK = 0,
    VW_ERR_NULL = 1,          /* NullPointerException                         */
    VW_ERR_EMPTY = 2,         /* VAL_006 VAL_EMPTY (empty signal / batch)     */
    VW_ERR_NONFINITE = 3,     /* VAL_003 VAL_NON_FINITE_VALUES; index via vw_last_error_index() */
    VW_ERR_LEVEL = 4,         /* CFG_004 CFG_INVALID_DECOMPOSITION_LEVEL      */
    VW_ERR_TOO_LARGE = 5,     /* VAL_005 VAL_TOO_LARGE (L_j > N)              */
    VW_ERR_BOUNDARY = 6,      /* CFG_003 CFG_UNSUPPORTED_BOUNDARY_MODE        */
    VW_ERR_ARG = 7,           /* IllegalArgumentException (shapes, ld, taps)  */
    VW_ERR_DEVICE = 8,        /* HIP runtime failure                          */
    VW_ERR_UNSUPPORTED = 9,   /* UnsupportedOperationException                */
    VW_ERR_STATE = 10         /* IllegalStateException (streaming)            */
};

/* BoundaryMode (core/api/BoundaryMode.java:20-50); CONSTANT is not a MODWT mode. */
enum { VW_PERIODIC = 0, VW_SYMMETRIC = 1, VW_ZERO_PADDING = 2 };

/* Wavelet identity for SymmetricAlignmentStrategy.decide, which compares
 * object identity (core/modwt/SymmetricAlignmentStrategy.java:65-96).
 * VW_WID_OTHER means "decide by filter length" (Haar if L <= 2, the L >= 12
 * rule, else the DB4 rule). */
enum {
    VW_WID_OTHER = 0, VW_WID_HAAR = 1, VW_WID_DB2 = 2, VW_WID_DB4 = 4, VW_WID_DB6 = 6,
    VW_WID_DB8 = 8, VW_WID_DB10 = 10, VW_WID_SYM4 = 104, VW_WID_SYM8 = 108,
    VW_WID_COIF1 = 201, VW_WID_COIF2 = 202, VW_WID_COIF3 = 203, VW_WID_COIF5 = 205
};

/* Semantics flags (OR-able). */
enum {
    /* MultiLevelMODWTTransform / SWT semantics: level cap 9 (calculateMaxLevels) and the
     * L_j > N guard.  Without it: BatchMODWT semantics (no cap, levels >= 1). */
    VW_FLAG_CORE_LEVELS = 1u << 0,
    /* Non-finite input check (ValidationUtils.validateFiniteValues) and result re-validation
     * (MODWTResultImpl ctor) -> VW_ERR_NONFINITE.  Fused into the kernels. */
    VW_FLAG_VALIDATE = 1u << 1,
    /* MultiLevelMODWTTransform.decompose PERIODIC dispatch: levels with N >= 1024 and
     * N/8 < L_j <= N/2 use WaveletOperations' FFT path, which zero-pads to nextPow2(N)
     * (core/modwt/MultiLevelMODWTTransform.java:734-742, core/util/FftHeuristics.java:30-34).
     * The engine computes that linear-over-nextPow2 convolution directly (no FFT). */
    VW_FLAG_FFT_SWITCH = 1u << 2,
    /* Fused multiply-add accumulation (faster; differs from the Java order by ~1 ulp per tap).
     * Default (flag clear) is EXACT: separate multiply and add in the reference's order,
     * bit-identical to vectorwave-core. */
    VW_FLAG_FMA = 1u << 3,
    /* All array arguments are host pointers (staged through the context workspace). */
    VW_FLAG_HOST_MEMORY = 1u << 4,
    /* Synchronize the context stream before returning. */
    VW_FLAG_SYNC = 1u << 5,
    /* Single-level inverse, SYMMETRIC: use MODWTTransform.inverseBatchOptimized's (t+l)
     * orientation (core/modwt/MODWTTransform.java:671-684) instead of inverse's (t-l). */
    VW_FLAG_BATCH_SYM_INVERSE = 1u << 6,
    /* Single-level forward: BatchSIMDMODWT.haarBatchMODWTSoA's hard-coded 0.5/-0.5 taps
     * (ext/extensions/modwt/BatchSIMDMODWT.java:86-140) when L == 2. */
    VW_FLAG_BATCH_HAAR = 1u << 7,
    /* The unvalidated callers' non-finite semantics (multi-level calls without VW_FLAG_VALIDATE):
     * the reference multiplies every tap of the upsampled filters, zeros included, so a NaN / +-Inf
     * turns each output whose window reaches it through a zero tap into NaN (0 * Inf)
     * -- BatchMODWT.multiLevelAoS (ext/extensions/modwt/BatchSIMDMODWT.java:384-424),
     * inverseMultiLevelAoS -> MultiLevelMODWTTransform.reconstruct (core/modwt/MultiLevelMODWTTransform.java
     * :339-349, :554-645), VectorWaveSwtAdapter.forwardParallel / inverse (core/swt/VectorWaveSwtAdapter.java
     * :210-335, :435-487).  With this flag every row where a level input holds a non-finite value (found
     * on the cascade's final output, a_J / y, which every such value reaches) is recomputed with the
     * reference's full-tap loops (exact arithmetic, also under VW_FLAG_FMA): NaN and +-Inf land exactly
     * where the reference puts them.  Costs one read of that output plane (none where the kernel probes
     * its own rows) and one fix-up launch.  Streaming
     * (vw_stream_*) ZERO / SYMMETRIC blocks and flushes are covered too: the history convolution
     * (BatchSIMDMODWT.generalBatchMODWTSoAWithScaledFiltersAndHistory :447-507) multiplies every tap, and
     * the recomputed rows rewrite the histories they leave for the next block. */
    VW_FLAG_REF_NONFINITE = 1u << 8,
    /* Financial and energy calls (vw_fin_*, vw_modwt_energy_f64, vw_energy_planes_f64): every sum may be a
     * wave / workgroup tree reduction instead of the reference's sequential loop.  Default (flag clear): one lane adds in index order, bit-identical to
     * com.morphiqlabs.financial; the dependent fp64 adds of that walk then bound the call.  The
     * convolution stays EXACT either way. */
    VW_FLAG_TREE_SUMS = 1u << 9
};

/* ---- arrays: alignment, leading dimensions, extents ----------------------
 * Every array argument needs only the alignment of its element type (8 bytes for double, 4 for float): a pointer
 * into the middle of a larger buffer is fine, e.g. an element offset into a Java primitive array.  The engine uses
 * 16-byte vector loads and stores where every array of a launch happens to be 16-byte aligned and the rows are whole
 * vectors, and element accesses otherwise; the results are the same bits either way.  Row inputs take any leading
 * dimension ldx >= N and are (B - 1) * ldx + N elements long: the last row has no padding.  Bytes outside
 * [row, row + N) of an input -- row padding, whatever precedes or follows the array -- are neither read into any
 * result nor checked by VW_FLAG_VALIDATE or VW_FLAG_REF_NONFINITE; they may hold anything, NaN included.  Inputs are
 * never written.  Outputs are written exactly over their documented extent, every element of it, and nothing
 * outside it (tests/test_gpu_footprint.py). */

/* ---- context ---------------------------------------------------------- */
VW_API vw_status vw_ctx_create(int device, vw_ctx **out);
VW_API vw_status vw_ctx_destroy(vw_ctx *ctx);
/* Use an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream. */
VW_API vw_status vw_ctx_set_stream(vw_ctx *ctx, void *hip_stream);
/* Enqueue on the device's null (legacy default) stream, e.g. torch's default stream (handle 0). */
VW_API vw_status vw_ctx_use_null_stream(vw_ctx *ctx);
VW_API void *vw_ctx_get_stream(vw_ctx *ctx);
/* Kernel-path switches of this context (A/B experiments, tests), named like the environment
 * variables read once at vw_ctx_create (VW_FORCE_TILED, VW_MULTI_TILE, VW_INV_BLK, VW_NV, ...);
 * value < 0 restores the default.  VW_ERR_ARG for an unknown name. */
VW_API vw_status vw_ctx_set_option(vw_ctx *ctx, const char *key, int value);
VW_API vw_status vw_ctx_synchronize(vw_ctx *ctx);
VW_API int vw_ctx_device(vw_ctx *ctx);

/* Thread-local message / index of the last failing call on this thread. */
VW_API const char *vw_last_error(void);
VW_API int64_t vw_last_error_index(void);
VW_API const char *vw_version(void);
/* Signal numbers in this thread's VW_ERR_NONFINITE messages count from `base`: a caller that splits one
 * batch into row chunks (the JNI AoS natives, jni/vectorwave_amd_jni.c) sets each chunk's first row so the
 * message names the batch's signal (AmdMultiLevelMODWT.decomposeBatch's contract); 0 restores. */
VW_API void vw_set_signal_base(int64_t base);

/* ---- bookkeeping (host only) ------------------------------------------ */
/* getMaximumLevels(N) for a base filter of length L: largest J <= 9 with (L-1)*2^(J-1)+1 <= N. */
VW_API int vw_max_levels(int64_t N, int L);
/* (L-1)*2^(level-1)+1 */
VW_API int64_t vw_upsampled_length(int L, int level);

/* ---- multi-level MODWT ------------------------------------------------- */
VW_API vw_status vw_modwt_forward_f64(vw_ctx *ctx, const double *x, int64_t B, int64_t N, int64_t ldx,
                                      const double *lo, const double *hi, int L, int wavelet_id,
                                      int boundary, int J, unsigned flags,
                                      double *details, double *approx);
VW_API vw_status vw_modwt_forward_f32(vw_ctx *ctx, const float *x, int64_t B, int64_t N, int64_t ldx,
                                      const double *lo, const double *hi, int L, int wavelet_id,
                                      int boundary, int J, unsigned flags,
                                      float *details, float *approx);

/* detail_mask bit (j-1) set = use d_j, clear = zero details at level j
 * (reconstructFromLevel / reconstructLevels / extractLevel); approx_zero = 1 starts from a
 * zero approximation.  details may be NULL when detail_mask == 0; approx may be NULL when
 * approx_zero == 1.  Plain reconstruct: detail_mask = ~0u, approx_zero = 0. */
VW_API vw_status vw_modwt_inverse_f64(vw_ctx *ctx, const double *details, const double *approx,
                                      int64_t B, int64_t N, const double *lo, const double *hi, int L,
                                      int wavelet_id, int boundary, int J, unsigned detail_mask,
                                      int approx_zero, unsigned flags, double *y);
VW_API vw_status vw_modwt_inverse_f32(vw_ctx *ctx, const float *details, const float *approx,
                                      int64_t B, int64_t N, const double *lo, const double *hi, int L,
                                      int wavelet_id, int boundary, int J, unsigned detail_mask,
                                      int approx_zero, unsigned flags, float *y);

/* ---- biorthogonal banks: two filter lengths -----------------------------------------------------
 * BiorthogonalSpline.BIOR1_1 .. BIOR6_8 and ReverseBiorthogonalSpline.RBIO1_1 .. RBIO6_8
 * (core/api/BiorthogonalSpline.java:304-339, ReverseBiorthogonalSpline.java:107-128): the low-pass has Llo
 * taps, the high-pass Lhi, 1 <= Llo, Lhi <= 64 (else VW_ERR_ARG).  The caller passes the ANALYSIS pair
 * (lowPassDecomposition / highPassDecomposition) to the forward calls and the SYNTHESIS pair
 * (lowPassReconstruction / highPassReconstruction) to the inverse calls; wavelet_id is VW_WID_OTHER for these
 * families.  Every other argument, the layouts and the flags VALIDATE / HOST_MEMORY / SYNC / FMA /
 * REF_NONFINITE are those of the equal-length calls, and with Llo == Lhi each call IS its equal-length
 * counterpart (same plan, same bits).  What the reference does with two lengths, restated:
 *   forward           each filter over its own upsampled length, ascending taps (:731-754).
 *   CORE_LEVELS       J > vw_max_levels(N, Llo) -> VW_ERR_LEVEL (the cap reads the low-pass alone, :455-501);
 *                     max(Llo_J, Lhi_J) > N -> VW_ERR_TOO_LARGE (:717-729, :561-574).  Without the flag: the
 *                     equal-length call's checks with L = max(Llo, Lhi).
 *   inverse PERIODIC  every low tap, then every high tap, one accumulator (:578-588).
 *   inverse SYMMETRIC decide() keys on Llo; the approximation branch shifts by tau(Llo) + dH, the detail
 *                     branch by tau(Lhi) + dG (:604-608).
 *   pairwise inverses (ZERO_PADDING multi-level :591-601; vw_modwt1_inverse in every mode, MODWTTransform.java
 *                     :203-299) loop over l < Llo_j and read high[l]: with Lhi >= Llo only the high taps
 *                     i < Llo are used (the reference's truncation); with Lhi < Llo the reference indexes past
 *                     its high-pass array (ArrayIndexOutOfBoundsException) -> VW_ERR_UNSUPPORTED.
 *   VW_FLAG_FFT_SWITCH the outer gate reads Llo_j, behind it each filter takes the FFT branch by its own
 *                     length (WaveletOperations.java:31-33).  A level of a non-power-of-two N >= 1024 where
 *                     exactly one filter does ("mixed level") is not implemented -> VW_ERR_UNSUPPORTED naming
 *                     the level; where both or neither do, the call runs as the equal-length one.
 * Without VW_FLAG_REF_NONFINITE, outputs whose window reaches a non-finite value are unspecified (the shorter
 * filter runs zero-extended: its absent taps multiply as zeros).  reconstructionScale / groupDelay are not
 * part of any MODWT path and are not applied.  Context option VW_BI (bit 0 forward, bit 1
 * inverse; 0 = neither): the fused kernels run each filter at its own tap count instead of zero-extending the
 * shorter one (same bits).  The default, 3, does so only for the pairs with compile-time kernels -- (9,7), (7,9),
 * (5,3), (3,5): bior4.4 / rbio4.4, bior2.2 / rbio2.2 -- and leaves EVERY OTHER PAIR on the zero-extended route;
 * bit 2 (VW_BI=7) runs those on the two-length runtime-tap bodies too, measured about 3 x slower than that route.
 * VW_BI_LISTED=0: the kernels run max(Llo, Lhi) taps
 * even where that count has no tap-unrolled kernels (default: one more zero tap where that reaches one; same bits). */
VW_API vw_status vw_modwt_forward_bi_f64(vw_ctx *ctx, const double *x, int64_t B, int64_t N, int64_t ldx,
                                         const double *lo, int Llo, const double *hi, int Lhi, int wavelet_id,
                                         int boundary, int J, unsigned flags, double *details, double *approx);
VW_API vw_status vw_modwt_forward_bi_f32(vw_ctx *ctx, const float *x, int64_t B, int64_t N, int64_t ldx,
                                         const double *lo, int Llo, const double *hi, int Lhi, int wavelet_id,
                                         int boundary, int J, unsigned flags, float *details, float *approx);
VW_API vw_status vw_modwt_inverse_bi_f64(vw_ctx *ctx, const double *details, const double *approx, int64_t B,
                                         int64_t N, const double *lo, int Llo, const double *hi, int Lhi,
                                         int wavelet_id, int boundary, int J, unsigned detail_mask,
                                         int approx_zero, unsigned flags, double *y);
VW_API vw_status vw_modwt_inverse_bi_f32(vw_ctx *ctx, const float *details, const float *approx, int64_t B,
                                         int64_t N, const double *lo, int Llo, const double *hi, int Lhi,
                                         int wavelet_id, int boundary, int J, unsigned detail_mask,
                                         int approx_zero, unsigned flags, float *y);
/* single level (vw_modwt1_*): MODWTTransform.forward convolves each filter on its own; its inverse is pairwise */
VW_API vw_status vw_modwt1_forward_bi_f64(vw_ctx *ctx, const double *x, int64_t B, int64_t N, int64_t ldx,
                                          const double *lo, int Llo, const double *hi, int Lhi, int boundary,
                                          unsigned flags, double *approx, double *detail);
VW_API vw_status vw_modwt1_inverse_bi_f64(vw_ctx *ctx, const double *approx, const double *detail, int64_t B,
                                          int64_t N, const double *lo, int Llo, const double *hi, int Lhi,
                                          int boundary, unsigned flags, double *y);

/* ---- wavelet energy per level --------------------------------------------------------------------
 * MultiLevelMODWTResult.getApproximationEnergy / getDetailEnergyAtLevel / getRelativeEnergyDistribution
 * (core/modwt/MultiLevelMODWTResultImpl.java:91-139, computeEnergy :211-216; MutableMultiLevelMODWTResultImpl
 * .java:143-208) for a batch.  out is [J+1][B] (the memory kind of the other arrays): out[0][b] the approximation
 * energy of signal b, out[j][b] the detail energy of level j -- getRelativeEnergyDistribution's order.  fp64 only:
 * the reference's energies are double sums of double coefficients.
 *
 * vw_modwt_energy_f64 takes vw_modwt_forward_f64's arguments, makes the same checks with the same statuses and
 * vw_last_error_index(), and sums the squares of the coefficients that call produces with the same flags:
 *   default             `energy = 0.0; for c: energy += c * c` in index order, a rounded square then a rounded
 *                       add: without VW_FLAG_FMA the reference's decompose(...) + computeEnergy bit for bit.
 *                       Exactness costs the plane traffic: the forward writes its (J+1)*B*N coefficients into
 *                       the context workspace and vw_energy_planes_f64's chain walk reads them back.
 *   VW_FLAG_TREE_SUMS   per-thread partials and fixed-order wave / workgroup trees: deterministic (the same call
 *                       gives the same bits), within N * 2^-52 relative of the sequential sum.  Where the fused
 *                       forward's cascade fits (and without VALIDATE / REF_NONFINITE / an FFT-switch level) one
 *                       launch reads x once and writes only out: no coefficient goes to HBM.  Elsewhere the
 *                       forward into the workspace, then the tree sums over its planes.
 *   VW_FLAG_FMA         affects the convolution only.
 * vw_energy_planes_f64 sums planes already in memory (details [J][B][N], approx [B][N]; J = 0: approx alone,
 * details may be NULL); flags: TREE_SUMS, HOST_MEMORY, SYNC.
 * Without HOST_MEMORY / VALIDATE / SYNC both calls can be recorded into a vw_graph once a call of that shape
 * has run (the workspace grows outside a capture only).  Context option VW_ENERGY_FUSED=0 keeps
 * vw_modwt_energy_f64 off the fused kernel. */
VW_API vw_status vw_modwt_energy_f64(vw_ctx *ctx, const double *x, int64_t B, int64_t N, int64_t ldx,
                                     const double *lo, const double *hi, int L, int wavelet_id,
                                     int boundary, int J, unsigned flags, double *out);
VW_API vw_status vw_energy_planes_f64(vw_ctx *ctx, const double *details, const double *approx, int64_t B,
                                      int64_t N, int J, unsigned flags, double *out);

/* ---- multiresolution analysis ----------------------------------------------------------------------
 * The additive split x = S_J + D_1 + ... + D_J of a MODWT, every component time-aligned to the signal, for a batch
 * in one call.  out is [J+1][B][N] in getRelativeEnergyDistribution's order: out[0] the smooth (the approximation
 * alone, every detail zeroed), out[j] detail component j (d_j alone, the approximation zeroed).  Component c is by
 * definition vw_modwt_inverse_* with detail_mask = c ? 1u << (c-1) : 0 and approx_zero = (c != 0), i.e.
 * VectorWaveSwtAdapter.extractLevel(signal, J, c) (core/swt/VectorWaveSwtAdapter.java:576-598) /
 * MultiLevelMODWTTransform.reconstructLevels (core/modwt/MultiLevelMODWTTransform.java:398-446) with one level:
 * without VW_FLAG_FMA bit for bit that call's result in all three boundary modes.
 *
 * vw_mra_planes_* takes coefficient planes (details [J][B][N], approx [B][N]) and makes vw_modwt_inverse_*'s checks
 * with the same statuses and messages.  Flags: CORE_LEVELS, FMA, HOST_MEMORY, SYNC, VALIDATE, REF_NONFINITE.
 * vw_modwt_mra_* takes signals: vw_modwt_forward_*'s checks first, then the inverse's; it runs the forward into the
 * context workspace and the planes call on those coefficients.  VW_FLAG_FFT_SWITCH applies to its forward only.
 * out must not overlap details, approx or x.  Equal-length banks only.
 *
 * Where a row and the longest level's halos fit the GPU's LDS twice, one launch computes all J+1 components and
 * leaves out the branch passes over zeroed planes (which cannot change a finite sum: the same bits).  That needs
 * finite data, so with VW_FLAG_VALIDATE or VW_FLAG_REF_NONFINITE -- and for rows that do not fit, for shapes where
 * that kernel measured slower (long listed filters on aligned rows), or with the context option VW_MRA_FUSED=0 --
 * the call issues the J+1 masked inverses instead: the same results.  VW_MRA_FUSED=2: the one launch wherever it fits.
 * Without HOST_MEMORY / VALIDATE / SYNC both calls can be recorded into a vw_graph once a call of that shape has
 * run (the workspace grows outside a capture only). */
VW_API vw_status vw_mra_planes_f64(vw_ctx *ctx, const double *details, const double *approx, int64_t B, int64_t N,
                                   const double *lo, const double *hi, int L, int wavelet_id, int boundary, int J,
                                   unsigned flags, double *out);
VW_API vw_status vw_mra_planes_f32(vw_ctx *ctx, const float *details, const float *approx, int64_t B, int64_t N,
                                   const double *lo, const double *hi, int L, int wavelet_id, int boundary, int J,
                                   unsigned flags, float *out);
VW_API vw_status vw_modwt_mra_f64(vw_ctx *ctx, const double *x, int64_t B, int64_t N, int64_t ldx,
                                  const double *lo, const double *hi, int L, int wavelet_id, int boundary, int J,
                                  unsigned flags, double *out);
VW_API vw_status vw_modwt_mra_f32(vw_ctx *ctx, const float *x, int64_t B, int64_t N, int64_t ldx,
                                  const double *lo, const double *hi, int L, int wavelet_id, int boundary, int J,
                                  unsigned flags, float *out);

/* ---- continuous wavelet transform ------------------------------------------------------------------
 * CWTTransform.analyze (cwt/CWTTransform.java:71-79) for a batch of rows, table-driven: the caller tabulates the
 * wavelet per scale, the GPU computes
 *
 *   out[b][s][tau] = ( sum_{k=0}^{K_s-1} w_s[k] * ext(x_b, tau + o_s + k) ) / q_s ,   tau in [0, N)
 *
 * with k ascending and ONE accumulator that starts at +0.0, the real (taps_re) and imaginary (taps_im) sums
 * independent.  Without VW_FLAG_FMA multiply and add are separate roundings; with it each term is one fma.  The
 * division is one IEEE division per output.  Every tap multiplies its sample, also a non-finite one, as the
 * reference's loops do.
 *   direct branch  analyzeDirect (:120-169) / analyzeDirectComplex (:174-218), t = -H..H ascending:
 *                  w_s[k] = psi(-(k - H)/s) / sqrtScale, K_s = 2H + 1, o_s = -H, q_s = 1, ext = the padding strategy,
 *                  H = max(16, ceil(8 s bandwidth)) / 2 (:774-794).
 *   FFT branch     analyzeFFT (:223-318), real wavelets: w_s[k] = psi((k - H)/s), K_s = 2H + 1, o_s = +H (the
 *                  extraction at i + halfSupport, :304-311: the window is NOT centred), q_s = sqrtScale,
 *                  ext = VW_CWT_WRAP_ZERO with wrap = fftSize = nextPow2(N + maxSupport - 1) (:234-238).  The
 *                  result is that branch's exact sum; the reference's FFT differs from it by its own rounding
 *                  (~1e-15 relative).  Non-finite input is unspecified there: the reference's FFT spreads it over
 *                  every output.
 * scales[s] = {tap_begin, taps K_s, window_begin o_s, divisor q_s}: w_s[k] = taps_re[tap_begin + k] (and taps_im),
 * tables of ntaps doubles on the HOST whatever the flags (rounded to float once by the _f32 call, the divisor
 * too).  taps_im == NULL: real output, out_im is not written and may be NULL.  x is [B][ldx]; out_re / out_im are
 * [B][S][N].  ext: VW_CWT_ZERO / REFLECT / SYMMETRIC / PERIODIC exactly as getBoundaryValue (:354-396), its clamps
 * to N-1 and 0 for a window that overshoots by more than N included; VW_CWT_WRAP_ZERO reads index mod wrap, zero
 * on [N, wrap).
 * Flags: VW_FLAG_FMA, VW_FLAG_HOST_MEMORY, VW_FLAG_SYNC; any other is VW_ERR_ARG.
 * Errors, all before any device work: null pointers VW_ERR_NULL; B, N or S = 0 VW_ERR_EMPTY; ldx < N, K_s < 1, a
 * descriptor reaching outside [0, ntaps), q_s <= 0 (or NaN), |o_s| > 2^30, an unknown ext, wrap < 1 with
 * WRAP_ZERO -> VW_ERR_ARG; K_s > 16384 -> VW_ERR_UNSUPPORTED naming the scale.
 * The tables and descriptors are kept on the device between calls: a call with the same ones uploads nothing, and
 * only such a call can be recorded into a vw_graph (VW_ERR_STATE otherwise).  Timing family: "cwt". */
enum { VW_CWT_ZERO = 0, VW_CWT_REFLECT = 1, VW_CWT_SYMMETRIC = 2, VW_CWT_PERIODIC = 3, VW_CWT_WRAP_ZERO = 4 };
typedef struct vw_cwt_scale {
    int64_t tap_begin;
    int32_t taps;
    int32_t window_begin;
    double divisor;
} vw_cwt_scale;
VW_API vw_status vw_cwt_f64(vw_ctx *ctx, const double *x, int64_t B, int64_t N, int64_t ldx,
                            const vw_cwt_scale *scales, int S, const double *taps_re, const double *taps_im,
                            int64_t ntaps, int ext, int64_t wrap, unsigned flags, double *out_re, double *out_im);
VW_API vw_status vw_cwt_f32(vw_ctx *ctx, const float *x, int64_t B, int64_t N, int64_t ldx,
                            const vw_cwt_scale *scales, int S, const double *taps_re, const double *taps_im,
                            int64_t ntaps, int ext, int64_t wrap, unsigned flags, float *out_re, float *out_im);

/* ---- inverse continuous wavelet transform ----------------------------------------------------------
 * InverseCWT.reconstruct / reconstructBand (cwt/InverseCWT.java) for a batch of coefficient planes coef [B][S][ldc]
 * (what vw_cwt_* writes when ldc == N) into rows out [B][ldo], table-driven like vw_cwt_*.  scales[j] =
 * {tap_begin, taps K_j, window_begin o_j, plane, weight, scale}: descriptor j reads plane `plane` of every row, so a
 * band is a descriptor list over a subset of the planes, with no copy.  w_j[k] = taps[tap_begin + k], a table of
 * ntaps doubles on the HOST whatever the flags (rounded to float once by the _f32 call; weight, scale and divisor too).
 *
 *   VW_ICWT_SUM     out[b][tau] = ( sum_j weight_j * ( sum_{k=0}^{K_j-1} w_j[k] * z_{b,plane_j}[(tau + o_j + k) mod wrap] ) ) / divisor
 *                   z = the plane's row, zero on [N, wrap).  j ascends in descriptor order, k ascends; each descriptor has
 *                   its own accumulator started at +0.0, and one outer accumulator started at +0.0 takes
 *                   total = total + acc_j * weight_j.  Without VW_FLAG_FMA multiply and add are separate roundings,
 *                   inner and outer; with it each is one fma.  One IEEE division per output.  `scale` is not read.
 *                   This is the sum reconstructInternalRealFFT (:225-270, N >= 128) evaluates by FFT: with
 *                   g_j(d) = psi(d / a_j) / sqrt(a_j), d in (-M/2, M/2], cut to [d_min, d_max] at its outermost non-zero
 *                   entries: o_j = -d_max, w_j[k] = g_j(d_max - k), weight_j = weights[j] / a_j (divided in double,
 *                   :238), wrap = M = nextPowerOfTwo(N), divisor = C_psi.  The reference's FFT differs from the sum
 *                   by its own rounding.
 *   VW_ICWT_DIRECT  reconstructInternalRealDirect (:283-311, N < 128) literally, in the element type: per output t one
 *                   accumulator over the descriptors and b = 0..N-1 ascending,
 *                   sum += ((c * w_j[t - b + N - 1]) * weight_j) / scale_j with c = coef[b'][plane_j][b], terms with
 *                   fabs(c) < 1e-10 skipped (a NaN is not), then / divisor.  K_j = 2N - 1; o_j and wrap are not read.
 * Flags: VW_FLAG_FMA (SUM only), VW_FLAG_HOST_MEMORY, VW_FLAG_SYNC; any other is VW_ERR_ARG.
 * Errors, all before any device work: null pointers VW_ERR_NULL; B, S, N or nsc = 0 VW_ERR_EMPTY; ldc < N, ldo < N,
 * K_j < 1, a descriptor reaching outside [0, ntaps), plane outside [0, S), |o_j| > 2^30, divisor <= 0 (or NaN),
 * wrap < N in SUM, K_j != 2N - 1 or VW_FLAG_FMA in DIRECT, an unknown form -> VW_ERR_ARG; K_j > 16384 ->
 * VW_ERR_UNSUPPORTED naming the descriptor.
 * The table and descriptors are kept on the device between calls in a slot of their own (vw_cwt_* and vw_icwt_*
 * calls do not evict each other's): a call with the same ones uploads nothing, and only such a call can be
 * recorded into a vw_graph (VW_ERR_STATE otherwise).  Timing family: "icwt". */
enum { VW_ICWT_SUM = 0, VW_ICWT_DIRECT = 1 };
typedef struct vw_icwt_scale {
    int64_t tap_begin;
    int32_t taps;
    int32_t window_begin;
    int32_t plane;
    double weight;
    double scale;
} vw_icwt_scale;
VW_API vw_status vw_icwt_f64(vw_ctx *ctx, const double *coef, int64_t B, int S, int64_t N, int64_t ldc,
                             const vw_icwt_scale *scales, int nsc, const double *taps, int64_t ntaps, int form,
                             int64_t wrap, double divisor, unsigned flags, double *out, int64_t ldo);
VW_API vw_status vw_icwt_f32(vw_ctx *ctx, const float *coef, int64_t B, int S, int64_t N, int64_t ldc,
                             const vw_icwt_scale *scales, int nsc, const double *taps, int64_t ntaps, int form,
                             int64_t wrap, double divisor, unsigned flags, float *out, int64_t ldo);

/* ---- one batch over several contexts (one host thread per context) ----------------------------
 * Replaces the reference's in-process parallelism over one batch call: BatchMODWT.multiLevelAoS /
 * inverseMultiLevelAoS (ext/extensions/modwt/BatchMODWT.java:90-111, :151-178) and the
 * VectorWaveSwtAdapter executor (core/swt/VectorWaveSwtAdapter.java:210-267).  The B rows are split
 * into n contiguous blocks (the first B % n blocks one row longer; min(n, B) blocks), block k runs on
 * ctxs[k] from its own host thread (ctxs[0] on the calling thread); the call returns when every
 * block is done.  Contexts may live on different devices or share one.  flags must include
 * VW_FLAG_HOST_MEMORY: the arrays are the caller's host arrays, laid out as the single-context
 * calls (details [J][B][N]); each thread stages its block through its context.  Errors: the first
 * failing block's status; vw_last_error() names the block. */
VW_API vw_status vw_modwt_forward_multi_f64(vw_ctx *const *ctxs, int nctx, const double *x, int64_t B, int64_t N,
                                            int64_t ldx, const double *lo, const double *hi, int L, int wavelet_id,
                                            int boundary, int J, unsigned flags, double *details, double *approx);
VW_API vw_status vw_modwt_inverse_multi_f64(vw_ctx *const *ctxs, int nctx, const double *details,
                                            const double *approx, int64_t B, int64_t N, const double *lo,
                                            const double *hi, int L, int wavelet_id, int boundary, int J,
                                            unsigned detail_mask, int approx_zero, unsigned flags, double *y);

/* Device-resident form of the two calls above (each device has its own context,
 * stream, input and output buffers; one host thread per device): context k works on ITS OWN device
 * buffers -- x[k] is rows[k] x ldx on ctxs[k]'s device, details[k] is [J][rows[k]][N], approx[k] and
 * y[k] are [rows[k]][N] -- so an FFM / JNI caller that keeps one batch shard resident per GPU calls all
 * of them at once with no host staging.  Host thread k enqueues on ctxs[k]'s stream (ctxs[0] on the
 * calling thread); the call returns when every context's work is enqueued, or finished with
 * VW_FLAG_SYNC.  rows[k] = 0 skips context k.  VW_FLAG_HOST_MEMORY is refused (VW_ERR_ARG).  Errors:
 * the first failing context's status; vw_last_error() names the context.
 * Replaces: BatchMODWT.multiLevelAoS / inverseMultiLevelAoS (ext/extensions/modwt/BatchMODWT.java:90-111,
 * :151-178) over a batch already sharded across devices. */
VW_API vw_status vw_modwt_forward_multi_dev_f64(vw_ctx *const *ctxs, int nctx, const double *const *x,
                                                const int64_t *rows, int64_t N, int64_t ldx, const double *lo,
                                                const double *hi, int L, int wavelet_id, int boundary, int J,
                                                unsigned flags, double *const *details, double *const *approx);
VW_API vw_status vw_modwt_inverse_multi_dev_f64(vw_ctx *const *ctxs, int nctx, const double *const *details,
                                                const double *const *approx, const int64_t *rows, int64_t N,
                                                const double *lo, const double *hi, int L, int wavelet_id,
                                                int boundary, int J, unsigned detail_mask, int approx_zero,
                                                unsigned flags, double *const *y);

/* ---- single-level MODWT (MODWTTransform: pairwise inverse sums, any N >= 1) --- */
VW_API vw_status vw_modwt1_forward_f64(vw_ctx *ctx, const double *x, int64_t B, int64_t N, int64_t ldx,
                                       const double *lo, const double *hi, int L, int boundary,
                                       unsigned flags, double *approx, double *detail);
VW_API vw_status vw_modwt1_inverse_f64(vw_ctx *ctx, const double *approx, const double *detail,
                                       int64_t B, int64_t N, const double *lo, const double *hi, int L,
                                       int boundary, unsigned flags, double *y);

/* ---- financial analytics (com.morphiqlabs.financial) ---------------------------------------------
 * One fused launch per call: each row is read from HBM once, its returns and level-1 PERIODIC MODWT
 * coefficients live in LDS, and only the reduced doubles are written.  Row length (N - 1 returns for
 * analyze, N for the Sharpe calls) is at most 16384 (VW_ERR_UNSUPPORTED beyond, as SURE); L <= 30.
 * Flags: VW_FLAG_HOST_MEMORY, VW_FLAG_SYNC, VW_FLAG_VALIDATE, VW_FLAG_TREE_SUMS.  VW_FLAG_FMA is refused
 * (VW_ERR_ARG): real prices are quantised, so many level-1 details are exactly 0.0 in EXACT arithmetic and
 * the reference's `detail > 0 / < 0` classification counts them as neither; a fused multiply-add leaves a
 * rounding residue there, turning zeros into signed values and changing the counts, not just the last bit.
 * Without HOST_MEMORY / VALIDATE / SYNC the calls can be recorded into a vw_graph (nothing is allocated
 * after the first call of a shape). */

/* FinancialAnalyzer (fin/FinancialAnalyzer.java), transform fixed by the caller's taps (the reference uses
 * DB4), PERIODIC.  Per price row p[0..N): returns r[i] = (p[i+1]-p[i])/p[i] when |p[i]| > 1e-10 else 0.0
 * (calculateReturns :248-265), d / a = level-1 MODWT of r (vw_modwt1_forward_f64's EXACT arithmetic, any
 * n = N-1 >= 1), then out[0][b] analyzeCrashAsymmetry :52-91, out[1][b] analyzeVolatility :103-120,
 * out[2][b] analyzeRegimeTrend :132-154, out[3][b] detectAnomalies :166-198 with threshold anomaly_k (1.0 /
 * 0.0), out[4][b] the detail standard deviation detectAnomalies compares against.  out is [5][B].
 * Errors: N < 2 VW_ERR_ARG (validatePrices :270-276).  With VW_FLAG_VALIDATE: a non-finite price is
 * VW_ERR_ARG "Prices must contain only finite values" (:279-283), else a return that overflows to +-Inf
 * is VW_ERR_NONFINITE (transform.forward's validation); vw_last_error_index() = b*N + i of the first such
 * price p[i] (any non-finite price comes before any overflowed return), else of the first such return
 * r[i], b counted from vw_set_signal_base.  Without it such rows give unspecified values. */
VW_API vw_status vw_fin_analyze_f64(vw_ctx *ctx, const double *prices, int64_t B, int64_t N, int64_t ld,
                                    const double *lo, const double *hi, int L, double anomaly_k,
                                    unsigned flags, double *out);
/* FinancialWaveletAnalyzer.calculateSharpeRatio(returns, riskFreeRate) :95-124, :234-255 per row:
 * sequential mean, sequential sum of squared deviations, sample standard deviation (n - 1); a zero
 * deviation gives 0.0 when mean == risk_free, else +-Inf.  N == 0 VW_ERR_EMPTY, N == 1 VW_ERR_ARG. */
VW_API vw_status vw_fin_sharpe_f64(vw_ctx *ctx, const double *returns, int64_t B, int64_t N, int64_t ld,
                                   double risk_free, unsigned flags, double *out);
/* FinancialWaveletAnalyzer.calculateWaveletSharpeRatio(returns, riskFreeRate) :166-212: level-1 forward,
 * inverse with an all-zero detail array (bit-identical to vw_modwt1_inverse_f64 on a zero plane), then the
 * ratio above.  PERIODIC is one launch; ZERO_PADDING / SYMMETRIC run the single-level kernels in the
 * context workspace first.  N == 1 VW_ERR_ARG (the same check, reached after the transform);
 * VW_FLAG_VALIDATE: non-finite input VW_ERR_NONFINITE, as vw_modwt1_forward_f64. */
VW_API vw_status vw_fin_wavelet_sharpe_f64(vw_ctx *ctx, const double *returns, int64_t B, int64_t N, int64_t ld,
                                           const double *lo, const double *hi, int L, int boundary,
                                           double risk_free, unsigned flags, double *out);

/* ---- SWT denoise -------------------------------------------------------- */
/* threshold < 0: universal threshold sigma*sqrt(2 ln N), sigma = median(|d_1|)/0.6745 per signal;
 * threshold >= 0: that value on every detail level.  soft: 1 soft, 0 hard.
 * thresholds_out (optional, [B], same memory kind as y) receives the threshold used per signal. */
VW_API vw_status vw_swt_denoise_f64(vw_ctx *ctx, const double *x, int64_t B, int64_t N, int64_t ldx,
                                    const double *lo, const double *hi, int L, int wavelet_id,
                                    int boundary, int J, double threshold, int soft, unsigned flags,
                                    double *y, double *thresholds_out);
/* ---- AoS <-> SoA layout (BatchSIMDMODWT.convertToSoA / convertFromSoA) -- */
/* out[c][r] = in[r][c] for a rows x cols row-major matrix (out of place).  AoS double[B][N] -> the
 * facade's SoA double[N*B] (index t*B + b): rows = B, cols = N; back: rows = N, cols = B.
 * ext/extensions/modwt/BatchSIMDMODWT.java:282-308. */
VW_API vw_status vw_transpose_f64(vw_ctx *ctx, const double *in, int64_t rows, int64_t cols, unsigned flags,
                                  double *out);
VW_API vw_status vw_transpose_f32(vw_ctx *ctx, const float *in, int64_t rows, int64_t cols, unsigned flags,
                                  float *out);

/* ---- WaveletDenoiser ---------------------------------------------------- */
/* Replaces com.morphiqlabs.wavelet.denoising.WaveletDenoiser (core/denoising/WaveletDenoiser.java):
 *   levels == 0, method != FIXED : denoise(signal, method, type)            :124-143
 *   levels == 0, method == FIXED : denoiseFixed(signal, fixed_threshold, type) :354-364
 *   levels >= 1                  : denoiseMultiLevel(signal, levels, method, type) :155-170, with
 *                                  DenoisedMultiLevelResult's per-level thresholds :204-231
 *                                  (sigma = MAD(d_1)/0.6745, level j uses sigma / sqrt(2^j)).
 * method: VW_THR_* (calculateThreshold :394-436).  SURE needs N <= 16384 (VW_ERR_UNSUPPORTED).
 * soft: 1 SOFT, 0 HARD.  thresholds_out (optional, [max(levels,1)][B], same memory kind as y). */
#define VW_THR_UNIVERSAL 0
#define VW_THR_SURE 1
#define VW_THR_MINIMAX 2
#define VW_THR_BAYES 3
#define VW_THR_FIXED 4
VW_API vw_status vw_wavelet_denoise_f64(vw_ctx *ctx, const double *x, int64_t B, int64_t N, int64_t ldx,
                                        const double *lo, const double *hi, int L, int wavelet_id,
                                        int boundary, int levels, int method, double fixed_threshold, int soft,
                                        unsigned flags, double *y, double *thresholds_out);

/* sigma[b] = median(|coeffs[b][:]|) / 0.6745 (exact selection, even N = mean of middle pair). */
VW_API vw_status vw_noise_sigma_f64(vw_ctx *ctx, const double *coeffs, int64_t B, int64_t N,
                                    unsigned flags, double *sigma);
/* In-place soft/hard threshold of c[B][N] with per-signal thresholds thr[B] (device or host per flags). */
VW_API vw_status vw_threshold_f64(vw_ctx *ctx, double *c, int64_t B, int64_t N, const double *thr,
                                  int soft, unsigned flags);

/* ---- MODWTStreamingDenoiser statistics (device pointers only) ------------ */
/* core/modwt/streaming/MODWTStreamingDenoiser.java:133-272 with core/util/MathUtils.java:94-257.
 * median_out[b] = median(|x[b][:] - center[b]|) (center NULL: median(|x[b][:]|)), exact order
 * statistics, even N = mean of the middle pair (MathUtils.median); the two passes of
 * medianAbsoluteDeviation on non-negative data (any N; rows longer than 16384 with a center write the
 * deviations into a per-context scratch buffer first: it grows outside a capture only -- run such a
 * call once before recording it -- and never moves the workspace that recorded graphs use). */
VW_API vw_status vw_median_f64(vw_ctx *ctx, const double *x, int64_t B, int64_t N, const double *center,
                               unsigned flags, double *median_out);
/* out[0] = MathUtils.standardDeviation(x[0..N)) -- sequential sums, sqrt(ssd / (N-1)); N >= 2. */
VW_API vw_status vw_stddev_f64(vw_ctx *ctx, const double *x, int64_t N, unsigned flags, double *out);
/* updateNoiseEstimation's ring write: window[(start+k) % wsize] = |src[idx[k]]|, k < count <= wsize;
 * idx is a host array (the stratified sampling positions). */
VW_API vw_status vw_window_gather_abs_f64(vw_ctx *ctx, const double *src, const int32_t *idx, int64_t count,
                                          double *window, int64_t wsize, int64_t start);

/* ---- streaming (BatchStreamingMODWT) ------------------------------------ */
/* levels >= 1.  PERIODIC: every block independent (== vw_modwt_forward, no cap).
 * ZERO_PADDING / SYMMETRIC: per-level left history of L_j - 1 samples kept on the device. */
VW_API vw_status vw_stream_create(vw_ctx *ctx, const double *lo, const double *hi, int L,
                                  int boundary, int levels, vw_stream **out);
VW_API vw_status vw_stream_destroy(vw_stream *s);
/* block [B][n] -> details [levels][B][n], approx [B][n] (f64). */
VW_API vw_status vw_stream_process_f64(vw_stream *s, const double *block, int64_t B, int64_t n,
                                       unsigned flags, double *details, double *approx);
/* Synthetic tail of tail_len samples (ZERO/SYMMETRIC only); tail_len <= min history length. */
VW_API vw_status vw_stream_flush_f64(vw_stream *s, int64_t tail_len, unsigned flags,
                                     double *details, double *approx);
VW_API int64_t vw_stream_history_length(vw_stream *s, int level);
/* Batch of the last processed block (the rows a flush emits); -1 before the first block. */
VW_API int64_t vw_stream_batch(vw_stream *s);

/* ---- captured steps ------------------------------------------------------- */
/* A caller that repeats the same calls on the same buffers (a JNI server's per-batch loop, a
 * benchmark) records them once and replays them with one host call: host planning, argument
 * packing and the per-kernel launch cost are paid at capture.  Between vw_capture_begin and
 * vw_capture_end the context's calls are recorded (HIP stream capture of the context stream),
 * not run; calls that must synchronize (VW_FLAG_VALIDATE, VW_FLAG_HOST_MEMORY, VW_FLAG_SYNC, a
 * fixed denoise threshold, stream flush, workspace growth) fail with VW_ERR_STATE.  The context
 * must be bound to a stream other than the null stream.  No reference counterpart: the Java
 * callers re-enter per call; this is the device-side amortisation of that loop. */
typedef struct vw_graph vw_graph;
VW_API vw_status vw_capture_begin(vw_ctx *ctx);
VW_API vw_status vw_capture_end(vw_ctx *ctx, vw_graph **out);
/* Replays the recorded calls `count` times, in order, on the context's stream (asynchronous).
 * Timing enabled during the capture (vw_ctx_enable_timing) records every launch's HIP events as
 * event nodes of the graph; with timing enabled at launch, vw_ctx_kernel_time then reports the
 * launches of the last replay of the call. */
VW_API vw_status vw_graph_launch(vw_graph *graph, int64_t count);
VW_API vw_status vw_graph_destroy(vw_graph *graph);
/* What a capture recorded: the graph's kernel nodes, and how many forward -> inverse pairs became one
 * round-trip launch (below; each counts one kernel node).  Either pointer may be NULL. */
VW_API vw_status vw_graph_stats(vw_graph *graph, int *kernel_nodes, int *fused_pairs);

/* ---- forward + inverse of the same rows in one launch --------------------------------------------
 * vw_modwt_forward_f64(x -> details, approx) followed by vw_modwt_inverse_f64(details, approx -> y, every level
 * kept): the same arrays, bit for bit, in both accumulation modes.  Where the pair is eligible -- device memory,
 * fp64, PERIODIC, a filter of at most 8 taps, rows the persistent forward takes whole (N a multiple of 512
 * samples up to 4096), no VALIDATE / REF_NONFINITE, y apart from x / details / approx -- one kernel runs both
 * halves per row, keeps a_J and d_J (and up to two more detail rows, below) in registers and reads the other detail
 * rows back right after storing them;
 * otherwise the two kernels run.  lo / hi: the
 * analysis pair, rlo / rhi: the synthesis pair, L taps each.
 * While a context is capturing (vw_capture_begin), a vw_modwt_forward_f64 directly followed by its
 * vw_modwt_inverse_f64 is recorded as this one launch too (switch VW_PAIR_FUSE, 0 = off; never with timing
 * enabled: the per-kernel event nodes keep the two kernels). */
VW_API vw_status vw_modwt_roundtrip_f64(vw_ctx *ctx, const double *x, int64_t B, int64_t N, int64_t ldx,
                                        const double *lo, const double *hi, const double *rlo, const double *rhi,
                                        int L, int wavelet_id, int boundary, int J, unsigned flags, double *details,
                                        double *approx, double *y);
/* Resident workgroups per compute unit of that launch for rows of N samples (0: the shape is not eligible). */
VW_API vw_status vw_roundtrip_occupancy(vw_ctx *ctx, int64_t N, int L, int J, unsigned flags, int *per_cu);
/* The kernel keeps up to two more detail rows (d_{J-1}, d_{J-2}) in registers instead of reading them back: switch
 * VW_PAIR_KEEP = 0 | 1 | 2 forces that many; unset or negative, the context takes the most that cost no resident
 * workgroup.  Reports what a launch for rows of N samples on this context would run: *keep, the number of kept rows,
 * and *per_cu as vw_roundtrip_occupancy does (both 0: the shape is not eligible).  The arrays are the same bit for
 * bit whichever runs. */
VW_API vw_status vw_roundtrip_variant(vw_ctx *ctx, int64_t N, int L, int J, unsigned flags, int *keep, int *per_cu);

/* ---- pipelined round trips ---------------------------------------------------
 * A caller that runs forward + inverse over successive batches (a server's per-batch loop over
 * BatchMODWT.multiLevelAoS then inverseMultiLevelAoS, ext/extensions/modwt/BatchMODWT.java:90-111,
 * :151-178; the blocks of BatchStreamingMODWT) keeps R >= 2 device buffer sets and lets the engine
 * issue the steps: step i works on set i mod R, its forward on fwd_ctx's stream, then (event) its
 * inverse on inv_ctx's stream; step i's forward waits for step i - R's inverse.  Step i + 1's forward
 * thus overlaps step i's inverse -- what keeps a small batch (<= 2 signals per CU) from leaving the
 * GPU half idle at each pass's ends -- and the steps are issued from C++, not one host call per pass.
 * x[r] is [B][N] (ldx = N), details[r] [J][B][N], approx[r] and y[r] [B][N], elements of elem_bytes
 * (8: f64, 4: f32), all on the contexts' device (both contexts on one device; they may be the same
 * context, which serialises the steps).  flags: FMA / CORE_LEVELS; SYNC, VALIDATE and HOST_MEMORY are
 * refused (VW_ERR_ARG).  vw_pipeline_run enqueues `steps` steps and returns; vw_pipeline_join makes
 * fwd_ctx's stream wait for every enqueued inverse (then the next run starts with no pending edge).
 * Destroying a context kills its pipelines (run / join then return VW_ERR_STATE; a destroy waits for a run
 * that is issuing its steps); run / join while either context is capturing return VW_ERR_STATE.  As for
 * every call, a context must not be destroyed while another thread still passes it in. */
typedef struct vw_pipeline vw_pipeline;
VW_API vw_status vw_pipeline_create(vw_ctx *fwd_ctx, vw_ctx *inv_ctx, int elem_bytes, int sets, void *const *x,
                                    void *const *details, void *const *approx, void *const *y, int64_t B,
                                    int64_t N, const double *lo, const double *hi, int L, int wavelet_id,
                                    int boundary, int J, unsigned flags, vw_pipeline **out);
VW_API vw_status vw_pipeline_run(vw_pipeline *p, int64_t steps);
VW_API vw_status vw_pipeline_join(vw_pipeline *p);
/* buffer set of the most recently enqueued step (-1 before the first) */
VW_API int64_t vw_pipeline_last_set(vw_pipeline *p);
VW_API vw_status vw_pipeline_destroy(vw_pipeline *p);

/* ---- device utilities ---------------------------------------------------- */
/* x[i] = 2*u - 1 with u = (splitmix64(seed ^ (offset + i)) >> 11) * 2^-53. */
VW_API vw_status vw_fill_uniform_f64(vw_ctx *ctx, double *x, int64_t count, uint64_t seed, int64_t offset);
VW_API vw_status vw_fill_uniform_f32(vw_ctx *ctx, float *x, int64_t count, uint64_t seed, int64_t offset);
VW_API vw_status vw_device_alloc(vw_ctx *ctx, int64_t bytes, void **out);
VW_API vw_status vw_device_free(vw_ctx *ctx, void *p);
VW_API vw_status vw_memcpy(vw_ctx *ctx, void *dst, const void *src, int64_t bytes, int kind /*0 H2D,1 D2H,2 D2D*/);

/* Timing: average duration (ms) of the last `count` launches of the dominant kernel family
 * recorded with HIP events on the context stream when profiling is enabled. */
VW_API vw_status vw_ctx_enable_timing(vw_ctx *ctx, int enable);
VW_API vw_status vw_ctx_kernel_time(vw_ctx *ctx, const char *family, double *total_ms, int64_t *launches);
VW_API vw_status vw_ctx_reset_timing(vw_ctx *ctx);
/* Start / end (ms after ref_event, a hipEvent_t recorded earlier on any stream of the device) of the
 * timed launches of `family` not yet collected by vw_ctx_kernel_time: the wall window of a kernel
 * family when several contexts run concurrently.  *count = launches found (at most max written). */
VW_API vw_status vw_ctx_kernel_spans(vw_ctx *ctx, const char *family, void *ref_event, int64_t max,
                                     double *start_ms, double *end_ms, int64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* VECTORWAVE_AMD_H */
