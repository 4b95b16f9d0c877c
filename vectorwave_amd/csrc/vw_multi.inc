// vw_multi.inc -- launchers of the multi-level tile kernels (vw_dev_lvl.h k_forward_multi / k_inverse_multi),
// the tail of the instantiation unit vw_lvl.hip.  Grid: (tiles per signal, signals), 256 threads.
namespace vw {

template <typename T, bool INV>
static hipError_t dispatch_multi(const MultiArgs<T>& a, int lds, bool fma, hipStream_t st) {
  const dim3 grid((unsigned)((a.N + a.tile - 1) / a.tile), (unsigned)a.B), block(256);
  return dispatch_taps<Unlisted::kRuntimeL>(a.taps, fma, [&](auto l, auto m) {
    if constexpr (!INV) {
      return launch_k<k_forward_multi<T, l(), m()>>(grid, block, lds, st, a);
    } else {
      if constexpr (sizeof(T) == 8) {  // four output vectors per thread (host: vw_plan.cpp inverse_multi_layout)
        if (a.ni == 4) return launch_k<k_inverse_multi<T, l(), m(), 4>>(grid, block, lds, st, a);
      }
      return launch_k<k_inverse_multi<T, l(), m()>>(grid, block, lds, st, a);
    }
  });
}

template <typename T>
hipError_t launch_forward_multi(const MultiArgs<T>& a, int lds, bool fma, hipStream_t st) {
  return dispatch_multi<T, false>(a, lds, fma, st);
}
template <typename T>
hipError_t launch_inverse_multi(const MultiArgs<T>& a, int lds, bool fma, hipStream_t st) {
  return dispatch_multi<T, true>(a, lds, fma, st);
}
template hipError_t launch_forward_multi<VW_T>(const MultiArgs<VW_T>&, int, bool, hipStream_t);
template hipError_t launch_inverse_multi<VW_T>(const MultiArgs<VW_T>&, int, bool, hipStream_t);

}  // namespace vw
