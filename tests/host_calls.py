"""Every C-ABI entry point that accepts VW_FLAG_HOST_MEMORY, as one call on a `Side`: the same arguments with the
arrays in host memory (numpy, VW_FLAG_HOST_MEMORY) or on the device (torch, VW_FLAG_SYNC).  Shared by
test_gpu_host_staging.py (both sides give the same bits) and test_gpu_graph.py (the host side is refused while
capturing).  Inputs are fill_uniform(seed 42); row inputs have a leading dimension of N + 8 and are exactly
(B - 1) * ld + N elements long, the documented size."""
from ctypes import byref, c_void_p

import numpy as np

from oracle import oracle as O
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import BiorthogonalSpline, Daubechies

W = Daubechies.DB4
LO, HI = nat.taps_array(W.lowPassDecomposition()), nat.taps_array(W.highPassDecomposition())
RLO, RHI = nat.taps_array(W.lowPassReconstruction()), nat.taps_array(W.highPassReconstruction())
L = len(W.lowPassDecomposition())
# the _bi_ entry points: a bank of two lengths (5 / 3 taps)
BW = BiorthogonalSpline.BIOR2_2
BLO, BHI = nat.taps_array(BW.lowPassDecomposition()), nat.taps_array(BW.highPassDecomposition())
BRLO, BRHI = nat.taps_array(BW.lowPassReconstruction()), nat.taps_array(BW.highPassReconstruction())


class Side:
    def __init__(self, torch=None):
        self.torch = torch  # None: the host side
        self.flags = nat.FLAG_SYNC if torch else nat.FLAG_HOST_MEMORY
        self.keep, self.outs, self.handles = [], [], []

    def inp(self, a):
        a = np.ascontiguousarray(a).copy()
        if self.torch:
            a = self.torch.from_numpy(a).cuda()
        self.keep.append(a)
        return c_void_p(a.data_ptr() if self.torch else a.ctypes.data)

    def inout(self, a):
        p = self.inp(a)
        self.outs.append(self.keep[-1])
        return p

    def out(self, shape, dtype=np.float64):
        return self.inout(np.full(shape, np.nan, dtype))

    def close(self, lib):  # after the capture, if any, has ended (destroying a stream handle synchronizes)
        for h in self.handles:
            assert lib.vw_stream_destroy(h) == 0

    def results(self):
        if not self.torch:
            return self.outs
        self.torch.cuda.synchronize()
        return [t.cpu().numpy() for t in self.outs]


def u(count, dtype=np.float64):
    return O.fill_uniform(int(count), 42).astype(dtype)


def rows(B, N, dtype=np.float64):
    return u((B - 1) * (N + 8) + N, dtype)


def _forward(name, lo, hi, bi, dtype):
    def call(lib, ctx, s, B, N, J, bd):
        taps = (lo, len(lo), hi, len(hi)) if bi else (lo, hi, len(lo))
        return getattr(lib, name)(ctx, s.inp(rows(B, N, dtype)), B, N, N + 8, *taps, W.wavelet_id, bd, J, s.flags,
                                  s.out((J, B, N), dtype), s.out((B, N), dtype))
    return call


def _inverse(name, lo, hi, bi, dtype):
    def call(lib, ctx, s, B, N, J, bd):
        taps = (lo, len(lo), hi, len(hi)) if bi else (lo, hi, len(lo))
        return getattr(lib, name)(ctx, s.inp(u(J * B * N, dtype)), s.inp(u(B * N, dtype)), B, N, *taps, W.wavelet_id,
                                  bd, J, 0xFFFFFFFF, 0, s.flags, s.out((B, N), dtype))
    return call


def modwt1_forward(lib, ctx, s, B, N, J, bd):
    return lib.vw_modwt1_forward_f64(ctx, s.inp(rows(B, N)), B, N, N + 8, LO, HI, L, bd, s.flags, s.out((B, N)),
                                     s.out((B, N)))


def modwt1_inverse(lib, ctx, s, B, N, J, bd):
    return lib.vw_modwt1_inverse_f64(ctx, s.inp(u(B * N)), s.inp(u(B * N)), B, N, RLO, RHI, L, bd, s.flags,
                                     s.out((B, N)))


def energy(lib, ctx, s, B, N, J, bd):
    return lib.vw_modwt_energy_f64(ctx, s.inp(rows(B, N)), B, N, N + 8, LO, HI, L, W.wavelet_id, bd, J, s.flags,
                                   s.out((J + 1, B)))


def energy_planes(lib, ctx, s, B, N, J, bd):
    return lib.vw_energy_planes_f64(ctx, s.inp(u(J * B * N)), s.inp(u(B * N)), B, N, J, s.flags, s.out((J + 1, B)))


def mra_planes(lib, ctx, s, B, N, J, bd):
    return lib.vw_mra_planes_f64(ctx, s.inp(u(J * B * N)), s.inp(u(B * N)), B, N, RLO, RHI, L, W.wavelet_id, bd, J,
                                 s.flags, s.out((J + 1, B, N)))


def modwt_mra(lib, ctx, s, B, N, J, bd):
    return lib.vw_modwt_mra_f64(ctx, s.inp(rows(B, N)), B, N, N + 8, LO, HI, L, W.wavelet_id, bd, J, s.flags,
                                s.out((J + 1, B, N)))


def cwt(lib, ctx, s, B, N, J, bd):
    # one scale: db4's low-pass as the table, centred, on the periodic extension
    scale = (nat.CwtScale * 1)(nat.CwtScale(0, L, -(L // 2), 2.0))
    return lib.vw_cwt_f64(ctx, s.inp(rows(B, N)), B, N, N + 8, scale, 1, LO, None, L, nat.CWT_PERIODIC, 0, s.flags,
                          s.out((B, 1, N)), None)


def fin_analyze(lib, ctx, s, B, N, J, bd):
    # prices are positive: 2 + fill_uniform lies in [1, 3)
    return lib.vw_fin_analyze_f64(ctx, s.inp(rows(B, N) + 2.0), B, N, N + 8, LO, HI, L, 3.0, s.flags, s.out((5, B)))


def fin_sharpe(lib, ctx, s, B, N, J, bd):
    return lib.vw_fin_sharpe_f64(ctx, s.inp(rows(B, N)), B, N, N + 8, 0.01, s.flags, s.out((B,)))


def fin_wavelet_sharpe(lib, ctx, s, B, N, J, bd):
    return lib.vw_fin_wavelet_sharpe_f64(ctx, s.inp(rows(B, N)), B, N, N + 8, LO, HI, L, bd, 0.01, s.flags,
                                         s.out((B,)))


def noise_sigma(lib, ctx, s, B, N, J, bd):
    return lib.vw_noise_sigma_f64(ctx, s.inp(u(B * N)), B, N, s.flags, s.out((B,)))


def threshold(lib, ctx, s, B, N, J, bd):
    return lib.vw_threshold_f64(ctx, s.inout(u(B * N)), B, N, s.inp(np.full(B, 0.25)), 1, s.flags)


def transpose(lib, ctx, s, B, N, J, bd):
    return lib.vw_transpose_f64(ctx, s.inp(u(B * N)), B, N, s.flags, s.out((N, B)))


def swt_denoise(lib, ctx, s, B, N, J, bd):
    return lib.vw_swt_denoise_f64(ctx, s.inp(rows(B, N)), B, N, N + 8, LO, HI, L, W.wavelet_id, bd, J, -1.0, 1,
                                  s.flags, s.out((B, N)), s.out((B,)))


def wavelet_denoise(lib, ctx, s, B, N, J, bd):
    return lib.vw_wavelet_denoise_f64(ctx, s.inp(rows(B, N)), B, N, N + 8, LO, HI, L, W.wavelet_id, bd, J, 0, 0.0, 1,
                                      s.flags, s.out((B, N)), s.out((J, B)))


def stream_process(lib, ctx, s, B, N, J, bd):
    h = c_void_p()
    assert lib.vw_stream_create(ctx, LO, HI, L, bd, J, byref(h)) == 0
    s.handles.append(h)
    return lib.vw_stream_process_f64(h, s.inp(u(B * N)), B, N, s.flags, s.out((J, B, N)), s.out((B, N)))


# the entry points test_capture_refuses_synchronizing_calls adds to the multi-level forward and inverse
CAPTURE_CALLS = {
    "vw_modwt1_forward_f64": modwt1_forward, "vw_modwt1_inverse_f64": modwt1_inverse, "vw_modwt_energy_f64": energy,
    "vw_energy_planes_f64": energy_planes, "vw_mra_planes_f64": mra_planes, "vw_modwt_mra_f64": modwt_mra,
    "vw_cwt_f64": cwt, "vw_fin_analyze_f64": fin_analyze, "vw_fin_sharpe_f64": fin_sharpe,
    "vw_fin_wavelet_sharpe_f64": fin_wavelet_sharpe, "vw_noise_sigma_f64": noise_sigma, "vw_threshold_f64": threshold,
    "vw_transpose_f64": transpose, "vw_swt_denoise_f64": swt_denoise, "vw_wavelet_denoise_f64": wavelet_denoise,
    "vw_stream_process_f64": stream_process,
}

CALLS = dict(CAPTURE_CALLS)
for _t, _dt in (("f64", np.float64), ("f32", np.float32)):
    CALLS[f"vw_modwt_forward_{_t}"] = _forward(f"vw_modwt_forward_{_t}", LO, HI, False, _dt)
    CALLS[f"vw_modwt_inverse_{_t}"] = _inverse(f"vw_modwt_inverse_{_t}", RLO, RHI, False, _dt)
    CALLS[f"vw_modwt_forward_bi_{_t}"] = _forward(f"vw_modwt_forward_bi_{_t}", BLO, BHI, True, _dt)
    CALLS[f"vw_modwt_inverse_bi_{_t}"] = _inverse(f"vw_modwt_inverse_bi_{_t}", BRLO, BRHI, True, _dt)
