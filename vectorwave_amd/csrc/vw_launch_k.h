// vw_launch_k.h -- how the .hip units launch: launch_k, keyed on the kernel, and the dispatch of a run-time tap
// count and accumulation mode to compile-time ones.  For hipcc only: no .cpp unit includes it.
#pragma once
#include "vw_launch.h"

#include <atomic>
#include <type_traits>

namespace vw {

// Raise a kernel's dynamic-LDS limit past the 64 KiB default once per kernel instantiation AND
// device (the attribute belongs to the device's copy of the function; a call per launch costs host
// time).  One LdsOnce per kernel: launch_k owns it (vw_pair.hip's table of prepared variants, which keeps
// run-time function pointers for capture, holds one per entry).  Several host threads (one per context,
// vw_modwt_*_multi_f64) may race here -- the attribute call is idempotent and the flag is atomic.
constexpr int kMaxDevices = 64;
struct LdsOnce {
  std::atomic<int> limit[kMaxDevices];  // zero-initialised as a static: the 64 KiB default applies
};
inline hipError_t set_lds(const void* k, int lds_bytes, LdsOnce* once, int want = kLdsBytes) {
  if (lds_bytes <= 64 * 1024) return hipSuccess;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
  std::atomic<int>* f = dev < kMaxDevices ? &once->limit[dev] : nullptr;
  if (f && f->load(std::memory_order_acquire) >= lds_bytes) return hipSuccess;
  if (want < lds_bytes) want = lds_bytes;
  hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, want);
  if (e != hipSuccess) return e;
  if (f) f->store(want, std::memory_order_release);
  return hipSuccess;
}

// Launch kernel K: its LDS limit first (the flag is K's own, so no launcher can pair a kernel with another's),
// then the launch and its status.  EXACT_LIMIT: raise the limit to `lds` instead of kLdsBytes, for a kernel that
// also has static LDS (k_sure_threshold).
template <auto K, bool EXACT_LIMIT = false>
hipError_t lds_limit_k(int lds) {  // on its own where the limit must stand before the launch (an occupancy query)
  static LdsOnce once;
  return set_lds(reinterpret_cast<const void*>(K), lds, &once, EXACT_LIMIT ? lds : kLdsBytes);
}
template <auto K, bool EXACT_LIMIT = false, typename... A>
hipError_t launch_k(dim3 grid, dim3 block, int lds, hipStream_t st, const A&... a) {
  hipError_t e = lds_limit_k<K, EXACT_LIMIT>(lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(K, grid, block, lds, st, a...);
  return hipGetLastError();
}

// f(std::bool_constant<FMA>) for the run-time accumulation mode.
template <typename F>
hipError_t with_fma(bool fma, F&& f) {
  return fma ? f(std::true_type{}) : f(std::false_type{});
}

// What a tap count outside VW_TAP_LIST (or above CAP) gets: the runtime-L body, f(L = 0), or an error status.
enum class Unlisted { kRuntimeL, kNotSupported, kInvalidValue, kInvalidConfiguration };

// f(std::integral_constant<int, L>, std::bool_constant<FMA>) for the listed tap count `taps` <= CAP.  Only the
// listed counts up to CAP (and L = 0 under kRuntimeL) are instantiated, in both accumulation modes.
template <Unlisted U, int CAP = kMaxTaps, typename F>
hipError_t dispatch_taps(int taps, bool fma, F&& f) {
  switch (taps) {
#define VW_TAP_CASE(n) \
    case n:            \
      if constexpr (n <= CAP) return with_fma(fma, [&](auto m) { return f(std::integral_constant<int, n>{}, m); }); \
      break;
    VW_TAP_LIST(VW_TAP_CASE)
#undef VW_TAP_CASE
    default: break;
  }
  if constexpr (U == Unlisted::kRuntimeL) return with_fma(fma, [&](auto m) { return f(std::integral_constant<int, 0>{}, m); });
  else return U == Unlisted::kNotSupported ? hipErrorNotSupported
            : U == Unlisted::kInvalidValue ? hipErrorInvalidValue : hipErrorInvalidConfiguration;
}

// Two-length banks: f(<L>, <LH>, <FMA>) for a pair of VW_TAP_PAIR_LIST when `unrolled`, else the runtime-L body
// with its two counts, f(<0>, <0>, <FMA>).
template <typename F>
hipError_t dispatch_tap_pair(bool unrolled, int taps, int taps_hi, bool fma, F&& f) {
  if (unrolled) {
#define VW_TAP_CASE(lo, hi) \
    if (taps == lo && taps_hi == hi) \
      return with_fma(fma, [&](auto m) { return f(std::integral_constant<int, lo>{}, std::integral_constant<int, hi>{}, m); });
    VW_TAP_PAIR_LIST(VW_TAP_CASE)
#undef VW_TAP_CASE
  }
  return with_fma(fma, [&](auto m) { return f(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, m); });
}

}  // namespace vw
