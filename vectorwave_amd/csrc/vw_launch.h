// vw_launch.h -- every launcher's declaration: what the host layer (vw_host.h) calls and the .hip units define.
// Host-safe: HIP's types and nothing that needs hipcc.  Each returns hipSuccess or the launch error.  The helpers the
// units launch with (launch_k, the tap dispatch) are in vw_launch_k.h, which no .cpp unit sees.
#pragma once
#include <hip/hip_runtime.h>
#include "vw_internal.h"
#include "vw_deep.h"

namespace vw {

int fused_max_threads();

// Fused kernels (vw_fwd.hip, vw_inv.hip)
template <typename T>
hipError_t launch_forward_fused(const FwdArgs<T>& a, int threads, int lds_bytes, bool fma, int nv, hipStream_t st);
template <typename T>
hipError_t launch_forward_persist(const FwdArgs<T>& a, int threads, int lds_bytes, bool fma, int nv, hipStream_t st);
template <typename T>
hipError_t launch_forward_blk(const FwdArgs<T>& a, int threads, int lds_bytes, bool fma, int nv, hipStream_t st);
template <typename T>
hipError_t launch_inverse_fused(const InvArgs<T>& a, int threads, int lds_bytes, bool fma, int nv, hipStream_t st);

// k_roundtrip (vw_pair.hip).  pair_prepare raises the kernel's dynamic-LDS limit and queries its occupancy (per_cu:
// resident workgroups per CU, may be null): neither can be recorded, so the executor calls it where an eligible
// forward runs uncaptured.  pair_launch_shape gives the launch of a prepared (taps, mode, threads, lds) -- the
// host function, the resident grid -- and false for one that is not prepared on the current device; it makes no
// call a capture forbids.  keep: Tuning::pair_keep, the requested number of kept detail planes (< 0: auto); both
// prepare every variant and choose by pair_keep_variant (vw_internal.h), and report the choice (variant / keep) with
// its resident workgroups per CU.
struct PairLaunch {
  const void* func;
  unsigned grid, threads, lds;
  int keep, per_cu;
};
hipError_t pair_prepare(int taps, bool fma, int threads, int lds_bytes, int keep, int* per_cu, int* variant);
bool pair_launch_shape(int taps, bool fma, int threads, int lds_bytes, int keep, long long B, int cus, PairLaunch* out);
hipError_t launch_roundtrip(const PairArgs<double>& a, const PairLaunch& l, hipStream_t st);

// Per-level path (vw_lvl.hip, vw_deep.hip)
template <typename T>
hipError_t launch_forward_level(const LevelArgs<T>& a, int lds_bytes, bool fma, hipStream_t st);
template <typename T>
hipError_t launch_inverse_level(const LevelArgs<T>& a, int lds_bytes, bool fma, hipStream_t st);
template <typename T>
hipError_t launch_forward_sweep(const LevelArgs<T>& a, bool fma, hipStream_t st);
template <typename T>
hipError_t launch_inverse_sweep(const LevelArgs<T>& a, bool fma, hipStream_t st);
template <typename T>
hipError_t launch_inverse_sweepg(const LevelArgs<T>& a, int levels, int ka, int R, bool fma, hipStream_t st);
template <typename T>
hipError_t launch_forward_multi(const MultiArgs<T>& a, int lds_bytes, bool fma, hipStream_t st);
template <typename T>
hipError_t launch_inverse_multi(const MultiArgs<T>& a, int lds_bytes, bool fma, hipStream_t st);
template <typename T>
hipError_t launch_deep(const DeepArgs<T>& a, int lds_bytes, bool fma, bool inverse, hipStream_t st);

// The reference's own arithmetic for rows holding non-finite values (vw_ref.hip)
template <typename T>
hipError_t launch_flag_nonfinite(const RefScan<T>& a, hipStream_t st);
template <typename T>
hipError_t launch_ref_cascade(const RefArgs<T>& a, int grid, bool inverse, hipStream_t st);

// Matrix-core fp32 kernels (vw_mfma.hip); mfma_supported / mfma_halo / mfma_region: vw_taps.h
hipError_t launch_forward_mfma(const FwdArgs<float>& a, int lds, hipStream_t st);
hipError_t launch_inverse_mfma(const InvArgs<float>& a, int lds, hipStream_t st);

// Financial analytics (vw_fin.hip)
hipError_t launch_fin_analyze(const FinArgs& a, hipStream_t st);
hipError_t launch_fin_sharpe(const FinArgs& a, hipStream_t st);

// Wavelet energy per level (vw_energy.hip)
hipError_t launch_energy_fused(const EnergyArgs& a, int threads, int lds_bytes, bool fma, int nv, int grid,
                               hipStream_t st);
// tree = false: the reference's sequential sum per row (one lane per row); true: a workgroup tree per row
hipError_t launch_energy_planes(const EnergyPlanesArgs& a, bool tree, int cus, hipStream_t st);

// Multiresolution analysis (vw_mra.hip), continuous wavelet transform (vw_cwt.hip)
template <typename T>
hipError_t launch_mra(const MraArgs<T>& a, int threads, int lds_bytes, bool fma, int nv, int grid, hipStream_t st);
template <typename T>
hipError_t launch_cwt(const CwtArgs<T>& a, int threads, int lds_bytes, bool cplx, bool fma, int grid, hipStream_t st);

// Inverse continuous wavelet transform (vw_icwt.hip): the SUM form by plan_icwt's shape, the DIRECT form one
// thread per output
template <typename T>
hipError_t launch_icwt(const IcwtArgs<T>& a, int threads, int lds_bytes, bool fma, int grid, hipStream_t st);
template <typename T>
hipError_t launch_icwt_direct(const IcwtArgs<T>& a, hipStream_t st);

// Streaming history, thresholds, statistics and utilities (vw_misc.hip)
template <typename T>
hipError_t launch_history_update(const T* level_in, long long ld_in, const T* old_hist, T* new_hist,
                                 long long B, int n, int hist_len, hipStream_t st);
hipError_t launch_level_threshold(const double* coeffs, long long level_stride, const double* sigma,
                                  const DenoiseConsts& k, long long B, int levels, double* thr, hipStream_t st);
hipError_t launch_noise_sigma(const double* coeffs, long long ld, long long B, int N, double scale_c,
                              double* sigma_out, double* thr_out, hipStream_t st);
// Exact median of |x - center| per row (center nullptr: of |x|); N <= 16384 when center is given.
hipError_t launch_median(const double* x, long long ld, long long B, int N, const double* center, double* median_out,
                         hipStream_t st);
// out[b][i] = |x[b*ld + i] - center[b]| (MathUtils.medianAbsoluteDeviation's deviations), for the
// centered median of rows longer than the register-keyed path holds.
hipError_t launch_abs_center(const double* x, long long ld, long long B, int N, const double* center, double* out,
                             hipStream_t st);
hipError_t launch_seq_std(const double* x, int n, double* out, hipStream_t st);
hipError_t launch_gather_abs(const double* src, const int* idx, int count, double* window, int wsize, int start,
                             hipStream_t st);
template <typename T>
hipError_t launch_transpose(const T* in, long long rows, long long cols, T* out, hipStream_t st);
template <typename T>
hipError_t launch_threshold(T* c, long long B, long long N, const T* thr, int soft, hipStream_t st);
template <typename T>
hipError_t launch_fill_uniform(T* x, long long count, unsigned long long seed, long long offset, hipStream_t st);
template <typename T>
hipError_t launch_single_haar_batch(const T* x, long long ldx, long long B, int N, T* approx, T* detail,
                                    hipStream_t st);

}  // namespace vw
