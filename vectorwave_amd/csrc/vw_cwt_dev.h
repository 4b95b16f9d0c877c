// vw_cwt_dev.h -- device helpers shared by the continuous wavelet transform (vw_cwt.hip) and its inverse
// (vw_icwt.hip): the extension read and the LDS layout of a staged tile.  For hipcc only.
#pragma once
#include "vw_launch_k.h"

namespace vw {

// CWTTransform.getBoundaryValue (:354-396) for every index, the in-range read (:147-149) included.
template <typename T>
__device__ __forceinline__ T cwt_ext(const T* __restrict__ x, long long i, int N, int ext, long long M) {
  if (ext == kCwtWrapZero) {
    long long m = i % M;
    if (m < 0) m += M;
    return m < N ? x[m] : T(0);
  }
  if (i >= 0 && i < N) return x[i];
  switch (ext) {
    case kCwtReflect: {
      long long r = i < 0 ? -i : 2LL * N - i - 2;
      if (i < 0 && r >= N) r = N - 1;
      if (i >= N && r < 0) r = 0;
      return x[r];
    }
    case kCwtSymmetric: {
      long long r = i < 0 ? -i - 1 : 2LL * N - i - 1;
      if (i < 0 && r >= N) r = N - 1;
      if (i >= N && r < 0) r = 0;
      return x[r];
    }
    case kCwtPeriodic: return x[((i % N) + N) % N];
    default: return T(0);
  }
}

// LDS element of staged element e: chunk q = e / NV as two 16-byte halves, half h of every chunk in plane h, so the
// 64 lanes of a wave read 64 consecutive 16-byte slots of one plane (no bank conflict; adjacent chunks in one
// array would put lanes l and l + 8 of a ds_read_b128 group on the same banks).
template <int NV>
__device__ __forceinline__ int cwt_slot(int e, int chunks) {
  constexpr int V = NV / 2;
  const int q = e / NV, c = e % NV;
  return ((c / V) * chunks + q) * V + c % V;
}

}  // namespace vw
