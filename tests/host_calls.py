"""Every C-ABI entry point that accepts VW_FLAG_HOST_MEMORY, as one call on a `Side`: the same arguments with the
arrays in host memory (numpy, VW_FLAG_HOST_MEMORY) or on the device (torch, VW_FLAG_SYNC).  Shared by
test_gpu_host_staging.py (both sides give the same bits), test_gpu_graph.py (the host side is refused while
capturing) and test_gpu_footprint.py (tests/guarded.py's GuardedSide: every array inside guard zones).  Inputs are
fill_uniform(seed 42); row inputs have a leading dimension of N + 8 unless the caller names one and are exactly
(B - 1) * ld + N elements long, the documented size.  Every builder takes the wavelet (`w`), the leading dimension
(`ld`) and extra flags (`flags`) as keywords; the defaults are db4, N + 8 and none."""
from ctypes import byref, c_void_p

import numpy as np

from oracle import oracle as O
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import BiorthogonalSpline, Daubechies

W = Daubechies.DB4
L = len(W.lowPassDecomposition())
# the _bi_ entry points: a bank of two lengths (5 / 3 taps)
BW = BiorthogonalSpline.BIOR2_2


class Bank:
    """A filter bank given as plain tap lists (synthetic filters): what the builders read of a wavelet."""

    def __init__(self, lo, hi, rlo=None, rhi=None, wavelet_id=0):
        self.lo, self.hi, self.rlo, self.rhi, self.wavelet_id = lo, hi, rlo or lo, rhi or hi, wavelet_id

    def lowPassDecomposition(self): return self.lo
    def highPassDecomposition(self): return self.hi
    def lowPassReconstruction(self): return self.rlo
    def highPassReconstruction(self): return self.rhi


class Side:
    def __init__(self, torch=None):
        self.torch = torch  # None: the host side
        self.flags = nat.FLAG_SYNC if torch else nat.FLAG_HOST_MEMORY
        self.keep, self.outs, self.handles, self.matrices = [], [], [], []

    def inp(self, a, name=None):
        a = np.ascontiguousarray(a).copy()
        if self.torch:
            a = self.torch.from_numpy(a).cuda()
        self.keep.append(a)
        return c_void_p(a.data_ptr() if self.torch else a.ctypes.data)

    def inout(self, a, name=None):
        p = self.inp(a)
        self.outs.append(self.keep[-1])
        return p

    def out(self, shape, dtype=np.float64, name=None):
        return self.inout(np.full(shape, np.nan, dtype))

    def rows(self, B, N, ld, dtype=np.float64, add=0.0, name=None):
        """Row input [B, N] at leading dimension ld: exactly (B - 1) * ld + N elements, the padding finite."""
        flat = rows(B, N, dtype, ld)
        if add:
            flat = flat + add
        self.matrices.append(np.stack([flat[b * ld:b * ld + N] for b in range(B)]))
        return self.inp(flat)

    def table(self, values, name=None):  # a host array of float64 the C side reads on the host (filter taps)
        t = nat.taps_array(values)
        self.keep.append(t)
        return t

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


def rows(B, N, dtype=np.float64, ld=None):
    ld = N + 8 if ld is None else ld
    return u((B - 1) * ld + N, dtype)


def _dec(s, w):
    lo, hi = w.lowPassDecomposition(), w.highPassDecomposition()
    assert len(lo) == len(hi)
    return s.table(lo, "lo"), s.table(hi, "hi"), len(lo)


def _rec(s, w):
    lo, hi = w.lowPassReconstruction(), w.highPassReconstruction()
    assert len(lo) == len(hi)
    return s.table(lo, "rlo"), s.table(hi, "rhi"), len(lo)


def _bank(s, lo, hi, bi):
    return (s.table(lo, "lo"), len(lo), s.table(hi, "hi"), len(hi)) if bi else (s.table(lo, "lo"), s.table(hi, "hi"),
                                                                                 len(lo))


def _forward(name, bi, dtype):
    def call(lib, ctx, s, B, N, J, bd, w=None, ld=None, flags=0):
        w = w or (BW if bi else W)
        ld = N + 8 if ld is None else ld
        taps = _bank(s, w.lowPassDecomposition(), w.highPassDecomposition(), bi)
        return getattr(lib, name)(ctx, s.rows(B, N, ld, dtype, name="x"), B, N, ld, *taps, w.wavelet_id, bd, J,
                                  s.flags | flags, s.out((J, B, N), dtype, name="details"),
                                  s.out((B, N), dtype, name="approx"))
    return call


def _inverse(name, bi, dtype):
    def call(lib, ctx, s, B, N, J, bd, w=None, ld=None, flags=0, det=None, app=None, detail_mask=0xFFFFFFFF,
             approx_zero=0):
        w = w or (BW if bi else W)
        taps = _bank(s, w.lowPassReconstruction(), w.highPassReconstruction(), bi)
        det = u(J * B * N, dtype) if det is None else det
        app = u(B * N, dtype) if app is None else app
        dp = s.inp(det, name="details")
        ap = None if (approx_zero and app is False) else s.inp(app, name="approx")  # app=False: approx = NULL
        return getattr(lib, name)(ctx, dp, ap, B, N, *taps, w.wavelet_id,
                                  bd, J, detail_mask, approx_zero, s.flags | flags, s.out((B, N), dtype, name="y"))
    return call


def modwt1_forward(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
    ld = N + 8 if ld is None else ld
    return lib.vw_modwt1_forward_f64(ctx, s.rows(B, N, ld, name="x"), B, N, ld, *_dec(s, w), bd, s.flags | flags,
                                     s.out((B, N), name="approx"), s.out((B, N), name="detail"))


def modwt1_inverse(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0, app=None, det=None):
    app = u(B * N) if app is None else app
    det = u(B * N) if det is None else det
    return lib.vw_modwt1_inverse_f64(ctx, s.inp(app, name="approx"), s.inp(det, name="detail"), B, N, *_rec(s, w), bd,
                                     s.flags | flags, s.out((B, N), name="y"))


def energy(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
    ld = N + 8 if ld is None else ld
    return lib.vw_modwt_energy_f64(ctx, s.rows(B, N, ld, name="x"), B, N, ld, *_dec(s, w), w.wavelet_id, bd, J,
                                   s.flags | flags, s.out((J + 1, B), name="energies"))


def energy_planes(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
    return lib.vw_energy_planes_f64(ctx, s.inp(u(J * B * N), name="details"), s.inp(u(B * N), name="approx"), B, N, J,
                                    s.flags | flags, s.out((J + 1, B), name="energies"))


def _mra_planes(name, dtype):
    def call(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
        return getattr(lib, name)(ctx, s.inp(u(J * B * N, dtype), name="details"), s.inp(u(B * N, dtype), name="approx"),
                                  B, N, *_rec(s, w), w.wavelet_id, bd, J, s.flags | flags,
                                  s.out((J + 1, B, N), dtype, name="out"))
    return call


def _modwt_mra(name, dtype):
    def call(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
        ld = N + 8 if ld is None else ld
        return getattr(lib, name)(ctx, s.rows(B, N, ld, dtype, name="x"), B, N, ld, *_dec(s, w), w.wavelet_id, bd, J,
                                  s.flags | flags, s.out((J + 1, B, N), dtype, name="out"))
    return call


mra_planes = _mra_planes("vw_mra_planes_f64", np.float64)
modwt_mra = _modwt_mra("vw_modwt_mra_f64", np.float64)


def cwt(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
    # one scale: db4's low-pass as the table, centred, on the periodic extension
    ld = N + 8 if ld is None else ld
    scale = (nat.CwtScale * 1)(nat.CwtScale(0, L, -(L // 2), 2.0))
    return lib.vw_cwt_f64(ctx, s.rows(B, N, ld, name="x"), B, N, ld, scale, 1, s.table(W.lowPassDecomposition()), None,
                          L, nat.CWT_PERIODIC, 0, s.flags | flags, s.out((B, 1, N), name="out_re"), None)


def fin_analyze(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
    # prices are positive: 2 + fill_uniform lies in [1, 3)
    ld = N + 8 if ld is None else ld
    return lib.vw_fin_analyze_f64(ctx, s.rows(B, N, ld, add=2.0, name="prices"), B, N, ld, *_dec(s, w), 3.0,
                                  s.flags | flags, s.out((5, B), name="out"))


def fin_sharpe(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
    ld = N + 8 if ld is None else ld
    return lib.vw_fin_sharpe_f64(ctx, s.rows(B, N, ld, name="returns"), B, N, ld, 0.01, s.flags | flags,
                                 s.out((B,), name="out"))


def fin_wavelet_sharpe(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
    ld = N + 8 if ld is None else ld
    return lib.vw_fin_wavelet_sharpe_f64(ctx, s.rows(B, N, ld, name="returns"), B, N, ld, *_dec(s, w), bd, 0.01,
                                         s.flags | flags, s.out((B,), name="out"))


def noise_sigma(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
    return lib.vw_noise_sigma_f64(ctx, s.inp(u(B * N), name="coeffs"), B, N, s.flags | flags, s.out((B,), name="sigma"))


def threshold(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
    return lib.vw_threshold_f64(ctx, s.inout(u(B * N), name="c"), B, N, s.inp(np.full(B, 0.25), name="thr"), 1,
                                s.flags | flags)


def _transpose(name, dtype):
    def call(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
        return getattr(lib, name)(ctx, s.inp(u(B * N, dtype), name="in"), B, N, s.flags | flags,
                                  s.out((N, B), dtype, name="out"))
    return call


transpose = _transpose("vw_transpose_f64", np.float64)


def swt_denoise(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
    ld = N + 8 if ld is None else ld
    return lib.vw_swt_denoise_f64(ctx, s.rows(B, N, ld, name="x"), B, N, ld, *_dec(s, w), w.wavelet_id, bd, J, -1.0, 1,
                                  s.flags | flags, s.out((B, N), name="y"), s.out((B,), name="thresholds"))


def wavelet_denoise(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0, method=0):
    ld = N + 8 if ld is None else ld
    return lib.vw_wavelet_denoise_f64(ctx, s.rows(B, N, ld, name="x"), B, N, ld, *_dec(s, w), w.wavelet_id, bd, J,
                                      method, 0.0, 1, s.flags | flags, s.out((B, N), name="y"),
                                      s.out((J, B), name="thresholds"))


def stream_process(lib, ctx, s, B, N, J, bd, w=W, ld=None, flags=0):
    h = c_void_p()
    assert lib.vw_stream_create(ctx, *_dec(s, w), bd, J, byref(h)) == 0
    s.handles.append(h)
    return lib.vw_stream_process_f64(h, s.inp(u(B * N), name="block"), B, N, s.flags | flags,
                                     s.out((J, B, N), name="details"), s.out((B, N), name="approx"))


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
    CALLS[f"vw_modwt_forward_{_t}"] = _forward(f"vw_modwt_forward_{_t}", False, _dt)
    CALLS[f"vw_modwt_inverse_{_t}"] = _inverse(f"vw_modwt_inverse_{_t}", False, _dt)
    CALLS[f"vw_modwt_forward_bi_{_t}"] = _forward(f"vw_modwt_forward_bi_{_t}", True, _dt)
    CALLS[f"vw_modwt_inverse_bi_{_t}"] = _inverse(f"vw_modwt_inverse_bi_{_t}", True, _dt)

# calls only test_gpu_footprint.py makes (no VW_FLAG_HOST_MEMORY pairing, or a dtype the staging test does not walk)
MORE_CALLS = {
    "vw_mra_planes_f32": _mra_planes("vw_mra_planes_f32", np.float32),
    "vw_modwt_mra_f32": _modwt_mra("vw_modwt_mra_f32", np.float32),
    "vw_transpose_f32": _transpose("vw_transpose_f32", np.float32),
}
