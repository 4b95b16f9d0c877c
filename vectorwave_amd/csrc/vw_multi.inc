// vw_multi.inc -- launchers of the multi-level tile kernels (vw_device.h k_forward_multi /
// k_inverse_multi), included by the instantiation unit vw_lvl.hip (built once per element type)
// after vw_launch.h (VW_TAP_LIST, set_lds).  Grid: (tiles per signal, signals), 256 threads.
namespace vw {

template <typename T, int L, bool FMA, bool INV>
static hipError_t run_multi(const MultiArgs<T>& a, int lds, hipStream_t st) {
  const unsigned tiles = (unsigned)((a.N + a.tile - 1) / a.tile);
  auto k = INV ? k_inverse_multi<T, L, FMA> : k_forward_multi<T, L, FMA>;
  static LdsOnce configured, configured4;
  LdsOnce* once = &configured;
  if constexpr (INV && sizeof(T) == 8) {
    if (a.ni == 4) {  // four output vectors per thread (host: vw_plan.cpp inverse_multi_layout)
      k = k_inverse_multi<T, L, FMA, 4>;
      once = &configured4;
    }
  }
  hipError_t e = set_lds(k, lds, once);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, dim3(tiles, (unsigned)a.B), dim3(256), lds, st, a);
  return hipGetLastError();
}

template <typename T, bool INV>
static hipError_t dispatch_multi(const MultiArgs<T>& a, int lds, bool fma, hipStream_t st) {
  switch (a.taps) {
#define VW_CASE(n) \
    case n: return fma ? run_multi<T, n, true, INV>(a, lds, st) : run_multi<T, n, false, INV>(a, lds, st);
    VW_TAP_LIST(VW_CASE)
#undef VW_CASE
    default:
      return fma ? run_multi<T, 0, true, INV>(a, lds, st) : run_multi<T, 0, false, INV>(a, lds, st);
  }
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
