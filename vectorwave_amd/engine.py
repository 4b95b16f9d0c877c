"""Device engine: one C-ABI context per GPU, array plumbing for numpy (host) and torch (device).

numpy inputs go through the engine's host-memory path (VW_FLAG_HOST_MEMORY: staged H2D, computed,
copied back -- what a JNI caller gets); torch CUDA tensors are passed as device pointers and the
work is enqueued on torch's current stream, so results stay resident in HBM.

Nothing here computes on the CPU: every transform is a call into libvectorwave_amd.so.
"""
from __future__ import annotations

import ctypes
import threading
from ctypes import byref, c_double, c_int64, c_void_p
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from .errors import InvalidArgumentException, raise_for_status

try:  # torch is plumbing only (device memory, streams); optional for host-memory use
    import torch
except Exception:  # pragma: no cover
    torch = None


def _is_device_tensor(a) -> bool:
    return torch is not None and isinstance(a, torch.Tensor) and a.is_cuda


def _one_length(lo, hi, what: str) -> int:
    """The tap count of a call whose ABI takes ONE length for both filters: the C side reads that many doubles of each
    array, so a bank of two lengths must not reach it."""
    if len(lo) != len(hi):
        raise InvalidArgumentException(f"{what} takes one filter length, got {len(lo)} low-pass and {len(hi)} "
                                       f"high-pass taps")
    return len(lo)


def _check(status: int) -> None:
    if status != 0:
        raise_for_status(status, nat.last_error(), nat.last_error_index())


class Engine:
    """Per-device context (vw_ctx).  ``Engine.get(device)`` returns the process-wide instance."""

    _instances = {}
    _lock = threading.Lock()

    def __init__(self, device: int = 0):
        self.lib = nat.load()
        self.device = device
        ctx = c_void_p()
        _check(self.lib.vw_ctx_create(device, byref(ctx)))
        self.ctx = ctx
        self._ext_stream = None
        self._keep = None   # during capture(): device tensors the recorded calls allocate or convert

    @classmethod
    def get(cls, device: Optional[int] = None) -> "Engine":
        if device is None:
            device = torch.cuda.current_device() if (torch is not None and torch.cuda.is_available()) else 0
        with cls._lock:
            eng = cls._instances.get(device)
            if eng is None:
                eng = cls(device)
                cls._instances[device] = eng
            return eng

    def close(self) -> None:
        """Destroy this context (vw_ctx_destroy: drains its stream, invalidates its graphs).  Not for the
        shared instance of ``Engine.get``."""
        if self.ctx:
            with Engine._lock:
                if Engine._instances.get(self.device) is self:
                    del Engine._instances[self.device]
            _check(self.lib.vw_ctx_destroy(self.ctx))
            self.ctx = None

    # -- streams ------------------------------------------------------------------------------
    def bind_torch_stream(self) -> None:
        """Enqueue on torch's current stream of this device (orders engine work with torch ops)."""
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._ext_stream:
            # torch's default stream has handle 0 (the null stream), which vw_ctx_set_stream would read
            # as "use your own stream" -- unordered with torch's work
            _check(self.lib.vw_ctx_use_null_stream(self.ctx) if s == 0 else
                   self.lib.vw_ctx_set_stream(self.ctx, c_void_p(s)))
            self._ext_stream = s

    def set_option(self, key: str, value: int) -> None:
        """Kernel-path switch of this context (vw_ctx_set_option); value < 0 = default."""
        _check(self.lib.vw_ctx_set_option(self.ctx, key.encode(), int(value)))

    def options(self, **kv):
        """Context manager: set switches (VW_... = int) for the block, restore the defaults after."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            for k, v in kv.items():
                self.set_option(k, v)
            try:
                yield self
            finally:
                for k in kv:
                    self.set_option(k, -1)
        return cm()

    def synchronize(self) -> None:
        _check(self.lib.vw_ctx_synchronize(self.ctx))

    def enable_timing(self, on: bool = True) -> None:
        _check(self.lib.vw_ctx_enable_timing(self.ctx, 1 if on else 0))

    def reset_timing(self) -> None:
        _check(self.lib.vw_ctx_reset_timing(self.ctx))

    def kernel_time(self, family: str) -> Tuple[float, int]:
        ms = c_double()
        n = c_int64()
        _check(self.lib.vw_ctx_kernel_time(self.ctx, family.encode(), byref(ms), byref(n)))
        return ms.value, n.value

    def kernel_spans(self, family: str, ref_event, max_n: int = 4096):
        """[(start_ms, end_ms)] of the uncollected timed launches of `family`, relative to `ref_event`
        (a torch.cuda.Event recorded before them); call before kernel_time (vw_ctx_kernel_spans)."""
        st = (c_double * max_n)()
        en = (c_double * max_n)()
        n = c_int64()
        _check(self.lib.vw_ctx_kernel_spans(self.ctx, family.encode(), c_void_p(ref_event.cuda_event), max_n, st, en,
                                            byref(n)))
        return [(st[i], en[i]) for i in range(min(n.value, max_n))]

    # -- array helpers ------------------------------------------------------------------------
    def _prep(self, x, dtype=None):
        """Returns (array, is_device, ptr, dtype_is_f32)."""
        if _is_device_tensor(x):
            # an f64-only entry point (dtype=float64) must never get an f32 buffer: the kernel would
            # read and write 8-byte elements over a 4-byte allocation
            if dtype is not None:
                want = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
                if x.dtype != want:
                    x = x.to(want)
            elif x.dtype not in (torch.float64, torch.float32):
                x = x.to(torch.float64)
            if not x.is_contiguous():
                x = x.contiguous()
            if x.device.index != self.device:
                raise ValueError(f"tensor on cuda:{x.device.index}, engine on cuda:{self.device}")
            self.bind_torch_stream()
            if self._keep is not None:
                self._keep.append(x)   # a recorded graph reads this storage on every replay
            return x, True, c_void_p(x.data_ptr()), x.dtype == torch.float32
        if torch is not None and isinstance(x, torch.Tensor):
            x = x.detach().numpy()
        a = np.asarray(x)
        if dtype is None:
            dtype = np.float32 if a.dtype == np.float32 else np.float64
        a = np.ascontiguousarray(a, dtype=dtype)
        return a, False, a.ctypes.data_as(c_void_p), a.dtype == np.float32

    def _empty(self, like, is_dev, shape):
        if is_dev:
            t = torch.empty(shape, dtype=like.dtype, device=like.device)
            if self._keep is not None:
                self._keep.append(t)   # a recorded graph writes this storage on every replay
            return t
        return np.empty(shape, dtype=like.dtype)

    @staticmethod
    def _ptr(a, is_dev):
        if a is None:
            return None
        return c_void_p(a.data_ptr()) if is_dev else a.ctypes.data_as(c_void_p)

    @staticmethod
    def _flags(flags: int, is_dev: bool) -> int:
        return flags if is_dev else flags | nat.FLAG_HOST_MEMORY

    # -- transforms ---------------------------------------------------------------------------
    def forward(self, x, lo: Sequence[float], hi: Sequence[float], wavelet_id: int, boundary: int, levels: int,
                flags: int):
        """Multi-level forward.  x: [N] or [B,N] -> (details [J,(B,)N], approx [(B,)N])."""
        xa, dev, xp, f32 = self._prep(x)
        one = xa.ndim == 1
        B, N = (1, xa.shape[0]) if one else xa.shape
        det = self._empty(xa, dev, (levels, N) if one else (levels, B, N))
        app = self._empty(xa, dev, (N,) if one else (B, N))
        if len(lo) != len(hi):  # a biorthogonal bank: the analysis pair (vw_modwt_forward_bi_*)
            fn = self.lib.vw_modwt_forward_bi_f32 if f32 else self.lib.vw_modwt_forward_bi_f64
            _check(fn(self.ctx, xp, B, N, N, nat.taps_array(lo), len(lo), nat.taps_array(hi), len(hi), wavelet_id,
                      boundary, levels, self._flags(flags, dev), self._ptr(det, dev), self._ptr(app, dev)))
            return det, app
        fn = self.lib.vw_modwt_forward_f32 if f32 else self.lib.vw_modwt_forward_f64
        _check(fn(self.ctx, xp, B, N, N, nat.taps_array(lo), nat.taps_array(hi), len(lo), wavelet_id, boundary,
                  levels, self._flags(flags, dev), self._ptr(det, dev), self._ptr(app, dev)))
        return det, app

    def inverse(self, details, approx, lo, hi, wavelet_id: int, boundary: int, levels: int, flags: int,
                detail_mask: int = 0xFFFFFFFF, approx_zero: bool = False, shape=None):
        ref = approx if approx is not None else details
        ra, dev, _, f32 = self._prep(ref)
        da = dp = None
        if details is not None:
            da, _, dp, _ = self._prep(details, np.float32 if f32 else np.float64)
        aa = ap = None
        if approx is not None:
            aa, _, ap, _ = self._prep(approx, np.float32 if f32 else np.float64)
        if shape is None:
            shape = tuple(aa.shape if aa is not None else da.shape[1:])
        one = len(shape) == 1
        B, N = (1, shape[0]) if one else shape
        y = self._empty(ra, dev, shape)
        if len(lo) != len(hi):  # a biorthogonal bank: the synthesis pair (vw_modwt_inverse_bi_*)
            fn = self.lib.vw_modwt_inverse_bi_f32 if f32 else self.lib.vw_modwt_inverse_bi_f64
            _check(fn(self.ctx, dp, ap, B, N, nat.taps_array(lo), len(lo), nat.taps_array(hi), len(hi), wavelet_id,
                      boundary, levels, detail_mask & 0xFFFFFFFF, 1 if approx_zero else 0, self._flags(flags, dev),
                      self._ptr(y, dev)))
            return y
        fn = self.lib.vw_modwt_inverse_f32 if f32 else self.lib.vw_modwt_inverse_f64
        _check(fn(self.ctx, dp, ap, B, N, nat.taps_array(lo), nat.taps_array(hi), len(lo), wavelet_id, boundary, levels,
                  detail_mask & 0xFFFFFFFF, 1 if approx_zero else 0, self._flags(flags, dev), self._ptr(y, dev)))
        return y

    def roundtrip(self, x, lo, hi, rlo, rhi, wavelet_id: int, boundary: int, levels: int, flags: int):
        """vw_modwt_roundtrip_f64: forward (lo, hi) then inverse (rlo, rhi) of x [B,N] (or [N]), float64 ->
        (details, approx, y), the arrays of ``forward`` followed by ``inverse`` bit for bit; one launch where the
        pair is eligible."""
        xa, dev, xp, _ = self._prep(x, np.float64)
        one = xa.ndim == 1
        B, N = (1, xa.shape[0]) if one else xa.shape
        det = self._empty(xa, dev, (levels, N) if one else (levels, B, N))
        app = self._empty(xa, dev, xa.shape)
        y = self._empty(xa, dev, xa.shape)
        L = _one_length(lo, hi, "roundtrip")
        if _one_length(rlo, rhi, "roundtrip") != L:
            raise InvalidArgumentException("roundtrip takes one filter length for both pairs")
        _check(self.lib.vw_modwt_roundtrip_f64(self.ctx, xp, B, N, N, nat.taps_array(lo), nat.taps_array(hi),
                                               nat.taps_array(rlo), nat.taps_array(rhi), L, wavelet_id, boundary,
                                               levels, self._flags(flags, dev), self._ptr(det, dev),
                                               self._ptr(app, dev), self._ptr(y, dev)))
        return det, app, y

    def roundtrip_occupancy(self, N: int, L: int, levels: int, flags: int = 0) -> int:
        """Resident workgroups per CU of the round-trip launch for rows of N samples (0: not eligible)."""
        from ctypes import c_int
        n = c_int()
        _check(self.lib.vw_roundtrip_occupancy(self.ctx, int(N), int(L), int(levels), int(flags), byref(n)))
        return n.value

    def roundtrip_variant(self, N: int, L: int, levels: int, flags: int = 0):
        """(kept detail planes, resident workgroups per CU) of the round-trip launch this context would make for
        rows of N samples: the VW_PAIR_KEEP variant that runs ((0, 0): not eligible)."""
        from ctypes import c_int
        keep, n = c_int(), c_int()
        _check(self.lib.vw_roundtrip_variant(self.ctx, int(N), int(L), int(levels), int(flags), byref(keep), byref(n)))
        return keep.value, n.value

    def forward1(self, x, lo, hi, boundary: int, flags: int):
        xa, dev, xp, f32 = self._prep(x, np.float64)
        one = xa.ndim == 1
        B, N = (1, xa.shape[0]) if one else xa.shape
        app = self._empty(xa, dev, xa.shape)
        det = self._empty(xa, dev, xa.shape)
        if len(lo) != len(hi):
            _check(self.lib.vw_modwt1_forward_bi_f64(self.ctx, xp, B, N, N, nat.taps_array(lo), len(lo),
                                                     nat.taps_array(hi), len(hi), boundary, self._flags(flags, dev),
                                                     self._ptr(app, dev), self._ptr(det, dev)))
            return app, det
        _check(self.lib.vw_modwt1_forward_f64(self.ctx, xp, B, N, N, nat.taps_array(lo), nat.taps_array(hi), len(lo),
                                              boundary, self._flags(flags, dev), self._ptr(app, dev),
                                              self._ptr(det, dev)))
        return app, det

    def inverse1(self, approx, detail, lo, hi, boundary: int, flags: int):
        aa, dev, ap, _ = self._prep(approx, np.float64)
        da, _, dp, _ = self._prep(detail, np.float64)
        one = aa.ndim == 1
        B, N = (1, aa.shape[0]) if one else aa.shape
        y = self._empty(aa, dev, aa.shape)
        if len(lo) != len(hi):
            _check(self.lib.vw_modwt1_inverse_bi_f64(self.ctx, ap, dp, B, N, nat.taps_array(lo), len(lo),
                                                     nat.taps_array(hi), len(hi), boundary, self._flags(flags, dev),
                                                     self._ptr(y, dev)))
            return y
        _check(self.lib.vw_modwt1_inverse_f64(self.ctx, ap, dp, B, N, nat.taps_array(lo), nat.taps_array(hi), len(lo),
                                              boundary, self._flags(flags, dev), self._ptr(y, dev)))
        return y

    def denoise(self, x, lo, hi, wavelet_id: int, boundary: int, levels: int, threshold: float, soft: bool,
                flags: int, want_thresholds: bool = False):
        xa, dev, xp, _ = self._prep(x, np.float64)
        one = xa.ndim == 1
        B, N = (1, xa.shape[0]) if one else xa.shape
        y = self._empty(xa, dev, xa.shape)
        thr = self._empty(xa, dev, (B,)) if want_thresholds else None
        _check(self.lib.vw_swt_denoise_f64(self.ctx, xp, B, N, N, nat.taps_array(lo), nat.taps_array(hi),
                                           _one_length(lo, hi, "denoise"),
                                           wavelet_id, boundary, levels, float(threshold), 1 if soft else 0,
                                           self._flags(flags, dev), self._ptr(y, dev), self._ptr(thr, dev)))
        return (y, thr) if want_thresholds else y

    def wavelet_denoise(self, x, lo, hi, wavelet_id: int, boundary: int, levels: int, method: int, fixed: float,
                        soft: bool, flags: int, want_thresholds: bool = False):
        """vw_wavelet_denoise_f64 (WaveletDenoiser); thresholds [max(levels,1), B]."""
        xa, dev, xp, _ = self._prep(x, np.float64)
        one = xa.ndim == 1
        B, N = (1, xa.shape[0]) if one else xa.shape
        y = self._empty(xa, dev, xa.shape)
        thr = self._empty(xa, dev, (max(levels, 1), B)) if want_thresholds else None
        _check(self.lib.vw_wavelet_denoise_f64(self.ctx, xp, B, N, N, nat.taps_array(lo), nat.taps_array(hi),
                                               _one_length(lo, hi, "wavelet_denoise"),
                                               wavelet_id, boundary, levels, method, float(fixed), 1 if soft else 0,
                                               self._flags(flags, dev), self._ptr(y, dev), self._ptr(thr, dev)))
        return (y, thr) if want_thresholds else y

    # -- financial analytics (vw_fin_*) -----------------------------------------------------------
    def _rows(self, x, N):
        """(array, is_dev, ptr, B, N, ld) of a [N] / [B,ld] float64 input; ``N`` < ld: only the first N columns of
        each row are data (a non-contiguous leading dimension)."""
        xa, dev, xp, _ = self._prep(x, np.float64)
        B, ld = (1, xa.shape[0]) if xa.ndim == 1 else xa.shape
        n = ld if N is None else int(N)
        if n > ld:
            raise ValueError(f"N={n} exceeds the row width {ld}")
        return xa, dev, xp, B, n, ld

    def fin_analyze(self, prices, lo, hi, anomaly_k: float, flags: int = 0, N: Optional[int] = None):
        """vw_fin_analyze_f64: prices [N] or [B,N] -> [5,B] (asymmetry, volatility, regimeTrend, anomaly flag,
        detail std).  ``N``: row length when the array is wider (its width is the leading dimension)."""
        xa, dev, xp, B, n, ld = self._rows(prices, N)
        out = self._empty(xa, dev, (5, B))
        _check(self.lib.vw_fin_analyze_f64(self.ctx, xp, B, n, ld, nat.taps_array(lo), nat.taps_array(hi),
                                           _one_length(lo, hi, "fin_analyze"),
                                           float(anomaly_k), self._flags(flags, dev), self._ptr(out, dev)))
        return out

    def fin_sharpe(self, returns, risk_free: float, flags: int = 0, N: Optional[int] = None):
        """vw_fin_sharpe_f64: returns [N] or [B,N] -> [B]."""
        xa, dev, xp, B, n, ld = self._rows(returns, N)
        out = self._empty(xa, dev, (B,))
        _check(self.lib.vw_fin_sharpe_f64(self.ctx, xp, B, n, ld, float(risk_free), self._flags(flags, dev),
                                          self._ptr(out, dev)))
        return out

    def fin_wavelet_sharpe(self, returns, lo, hi, boundary: int, risk_free: float, flags: int = 0,
                           N: Optional[int] = None):
        """vw_fin_wavelet_sharpe_f64: returns [N] or [B,N] -> [B]."""
        xa, dev, xp, B, n, ld = self._rows(returns, N)
        out = self._empty(xa, dev, (B,))
        _check(self.lib.vw_fin_wavelet_sharpe_f64(self.ctx, xp, B, n, ld, nat.taps_array(lo), nat.taps_array(hi),
                                                  _one_length(lo, hi, "fin_wavelet_sharpe"), int(boundary),
                                                  float(risk_free), self._flags(flags, dev), self._ptr(out, dev)))
        return out

    # -- wavelet energy per level (vw_modwt_energy_f64 / vw_energy_planes_f64) ---------------------
    def energy(self, x, lo: Sequence[float], hi: Sequence[float], wavelet_id: int, boundary: int, levels: int,
               flags: int = 0, N: Optional[int] = None):
        """Energies of the multi-level forward of x [N] or [B,N] -> [J+1, B]: row 0 the approximation energy, row j
        the detail energy of level j.  Default: the reference's sequential ``energy += c * c`` bit for bit;
        FLAG_TREE_SUMS: tree sums, fused with the forward where its cascade fits (no coefficient leaves the GPU's
        LDS).  ``N``: row length when the array is wider (its width is the leading dimension)."""
        xa, dev, xp, B, n, ld = self._rows(x, N)
        out = self._empty(xa, dev, (levels + 1, B))
        _check(self.lib.vw_modwt_energy_f64(self.ctx, xp, B, n, ld, nat.taps_array(lo), nat.taps_array(hi),
                                            _one_length(lo, hi, "energy"),
                                            wavelet_id, boundary, levels, self._flags(flags, dev),
                                            self._ptr(out, dev)))
        return out

    def energy_planes(self, details, approx, flags: int = 0):
        """Energies of coefficient planes: details [J,B,N] (or [J,N]; None = no levels), approx [B,N] (or [N])
        -> [J+1, B] in [approx, d1..dJ] order."""
        aa, dev, ap, _ = self._prep(approx, np.float64)
        B, N = (1, aa.shape[0]) if aa.ndim == 1 else aa.shape
        J, dp = 0, None
        if details is not None and details.shape[0] > 0:
            da, ddev, dp, _ = self._prep(details, np.float64)
            J = int(da.shape[0])
            if ddev != dev or tuple(da.shape[1:]) != tuple(aa.shape):
                raise ValueError("details must be [J] + approx.shape, in the same memory as approx")
        out = self._empty(aa, dev, (J + 1, B))
        _check(self.lib.vw_energy_planes_f64(self.ctx, dp, ap, B, N, J, self._flags(flags, dev),
                                             self._ptr(out, dev)))
        return out

    # -- multiresolution analysis (vw_mra_planes_* / vw_modwt_mra_*) -------------------------------
    def mra_planes(self, details, approx, lo: Sequence[float], hi: Sequence[float], wavelet_id: int, boundary: int,
                   flags: int = 0):
        """Every additive component of the coefficient planes details [J,B,N] (or [J,N]) and approx [B,N] (or [N])
        -> [J+1,(B,)N]: row 0 the smooth (approximation alone), row j detail component j (d_j alone) -- each the
        inverse with every other plane zeroed, bit for bit without FLAG_FMA.  One launch where the rows fit and the
        flags promise finite data (neither FLAG_VALIDATE nor FLAG_REF_NONFINITE), else the J+1 masked inverses."""
        aa, dev, ap, f32 = self._prep(approx)
        da, ddev, dp, _ = self._prep(details, np.float32 if f32 else np.float64)
        if ddev != dev or da.ndim != aa.ndim + 1 or tuple(da.shape[1:]) != tuple(aa.shape) or da.shape[0] < 1:
            raise ValueError("details must be [J] + approx.shape with J >= 1, in the same memory as approx")
        J = int(da.shape[0])
        B, N = (1, aa.shape[0]) if aa.ndim == 1 else aa.shape
        out = self._empty(aa, dev, (J + 1,) + tuple(aa.shape))
        fn = self.lib.vw_mra_planes_f32 if f32 else self.lib.vw_mra_planes_f64
        _check(fn(self.ctx, dp, ap, B, N, nat.taps_array(lo), nat.taps_array(hi), _one_length(lo, hi, "mra_planes"),
                  wavelet_id, boundary, J, self._flags(flags, dev), self._ptr(out, dev)))
        return out

    def mra(self, x, lo: Sequence[float], hi: Sequence[float], wavelet_id: int, boundary: int, levels: int,
            flags: int = 0):
        """Multi-level forward of x [N] or [B,N], then mra_planes on its coefficients -> [J+1,(B,)N].  The
        coefficients stay in the context workspace; FLAG_FFT_SWITCH applies to the forward only."""
        xa, dev, xp, f32 = self._prep(x)
        B, N = (1, xa.shape[0]) if xa.ndim == 1 else xa.shape
        out = self._empty(xa, dev, (levels + 1,) + tuple(xa.shape))
        fn = self.lib.vw_modwt_mra_f32 if f32 else self.lib.vw_modwt_mra_f64
        _check(fn(self.ctx, xp, B, N, N, nat.taps_array(lo), nat.taps_array(hi), _one_length(lo, hi, "mra"),
                  wavelet_id, boundary, levels, self._flags(flags, dev), self._ptr(out, dev)))
        return out

    # -- continuous wavelet transform (vw_cwt_*) ----------------------------------------------------
    def cwt(self, x, scales, taps_re, taps_im, ext: int, wrap: int = 0, flags: int = 0, N: Optional[int] = None):
        """out[b][s][tau] = (sum_k w_s[k] * ext(x_b, tau + o_s + k)) / q_s, k ascending.  x: [N] or [B, ld] (N: the
        row length when the rows carry padding, ld > N).  scales: a sequence of (tap_begin, taps, window_begin,
        divisor) into the flat float64 tables taps_re / taps_im (taps_im None: real output).  ext: nat.CWT_*; wrap:
        the period of CWT_WRAP_ZERO.  -> (re, im or None), each [(B,) S, N]."""
        xa, dev, xp, f32 = self._prep(x)
        one = xa.ndim == 1
        B, ld = (1, xa.shape[0]) if one else xa.shape
        N = ld if N is None else int(N)
        S = len(scales)
        desc = (nat.CwtScale * max(S, 1))()
        for i, (t0, k, o, q) in enumerate(scales):
            desc[i] = nat.CwtScale(int(t0), int(k), int(o), float(q))
        tre = np.ascontiguousarray(taps_re, dtype=np.float64)
        tim = None if taps_im is None else np.ascontiguousarray(taps_im, dtype=np.float64)
        if tim is not None and tim.shape != tre.shape:
            raise ValueError("taps_im must have the shape of taps_re")
        shape = (S, N) if one else (B, S, N)
        ore = self._empty(xa, dev, shape)
        oim = None if tim is None else self._empty(xa, dev, shape)
        dpp = ctypes.POINTER(c_double)
        fn = self.lib.vw_cwt_f32 if f32 else self.lib.vw_cwt_f64
        _check(fn(self.ctx, xp, B, N, ld, desc, S, tre.ctypes.data_as(dpp),
                  None if tim is None else tim.ctypes.data_as(dpp), tre.size, ext, wrap, self._flags(flags, dev),
                  self._ptr(ore, dev), self._ptr(oim, dev)))
        return ore, oim

    # -- inverse continuous wavelet transform (vw_icwt_*) -------------------------------------------
    def icwt(self, coef, scales, taps, form: int, wrap: int, divisor: float, flags: int = 0,
             N: Optional[int] = None, out=None):
        """Coefficient planes coef [S, ld] or [B, S, ld] (N: the row length when the rows carry padding, ld > N) ->
        [N] / [B, N].  scales: a sequence of (tap_begin, taps, window_begin, plane, weight, scale) into the flat
        float64 table ``taps``.  form nat.ICWT_SUM: out = (sum_j weight_j (sum_k w_j[k] z_plane_j[(tau + o_j + k) mod
        wrap])) / divisor; nat.ICWT_DIRECT: InverseCWT's direct loops.  out: an array [B, ldo] (ldo >= N) in coef's
        memory to write instead of a new one."""
        ca, dev, cp, f32 = self._prep(coef)
        if ca.ndim not in (2, 3):
            raise ValueError("coef must be [S, N] or [B, S, N]")
        one = ca.ndim == 2
        B, S, ld = (1,) + tuple(ca.shape) if one else tuple(ca.shape)
        N = ld if N is None else int(N)
        nsc = len(scales)
        desc = (nat.IcwtScale * max(nsc, 1))()
        for i, (t0, k, o, pl, wt, sc) in enumerate(scales):
            desc[i] = nat.IcwtScale(int(t0), int(k), int(o), int(pl), float(wt), float(sc))
        tab = np.ascontiguousarray(taps, dtype=np.float64)
        if out is None:
            res = self._empty(ca, dev, (N,) if one else (B, N))
            ldo = N
        else:
            res, odev, _, of32 = self._prep(out)
            if res is not out or odev != dev or of32 != f32:
                raise ValueError("out must be a contiguous array of coef's element type, in the same memory")
            ldo = int(res.shape[-1])
        fn = self.lib.vw_icwt_f32 if f32 else self.lib.vw_icwt_f64
        _check(fn(self.ctx, cp, B, S, N, ld, desc, nsc, tab.ctypes.data_as(ctypes.POINTER(c_double)), tab.size,
                  int(form), int(wrap), float(divisor), self._flags(flags, dev), self._ptr(res, dev), ldo))
        return res

    def transpose(self, a, rows: int, cols: int):
        """out[c][r] = a[r][c] (a: rows*cols elements, any shape) -> flat [cols*rows] array."""
        aa, dev, ap, f32 = self._prep(a)
        if (aa.numel() if dev else aa.size) != rows * cols:
            raise ValueError("transpose: size mismatch")
        out = self._empty(aa, dev, (rows * cols,))
        fn = self.lib.vw_transpose_f32 if f32 else self.lib.vw_transpose_f64
        _check(fn(self.ctx, ap, rows, cols, self._flags(0, dev), self._ptr(out, dev)))
        return out

    def noise_sigma(self, coeffs):
        ca, dev, cp, _ = self._prep(coeffs, np.float64)
        one = ca.ndim == 1
        B, N = (1, ca.shape[0]) if one else ca.shape
        sig = self._empty(ca, dev, (B,))
        _check(self.lib.vw_noise_sigma_f64(self.ctx, cp, B, N, self._flags(0, dev), self._ptr(sig, dev)))
        return sig

    def threshold_inplace(self, coeffs, thresholds, soft: bool):
        """In-place threshold of a device tensor or numpy array [B,N] (or [N]) with per-row thresholds."""
        ca, dev, cp, _ = self._prep(coeffs, np.float64)
        one = ca.ndim == 1
        B, N = (1, ca.shape[0]) if one else ca.shape
        ta, _, tp, _ = self._prep(thresholds, np.float64)
        _check(self.lib.vw_threshold_f64(self.ctx, cp, B, N, tp, 1 if soft else 0, self._flags(0, dev)))
        if ca is not coeffs:  # _prep made a converted / contiguous copy: write the result back in place
            if dev:
                coeffs.copy_(ca)
            else:
                np.copyto(coeffs, ca)
        return coeffs

    # -- captured steps (vw_capture_begin / vw_capture_end / vw_graph_launch) --------------------
    def capture(self, fn) -> "Graph":
        """Record the engine calls ``fn()`` makes (device tensors, no validation) into one HIP graph.
        The engine must be bound to a non-default torch stream (``bind_torch_stream``).

        Every device tensor the recorded calls allocate (outputs) or convert (inputs made contiguous /
        cast) is kept alive by the returned Graph, so the caching allocator never hands that storage to
        another tensor while replays still write it; ``Graph.result`` is ``fn()``'s return value, whose
        tensors every replay rewrites.  If ``fn()`` raises, the partial graph is destroyed."""
        self.bind_torch_stream()
        _check(self.lib.vw_capture_begin(self.ctx))
        self._keep = []
        done = False
        result = None
        try:
            result = fn()
            done = True
        finally:
            keep, self._keep = self._keep, None
            g = c_void_p()
            st = self.lib.vw_capture_end(self.ctx, byref(g))
            if not done and st == 0:
                self.lib.vw_graph_destroy(g)
        _check(st)
        return Graph(self, g, keep=keep, result=result)

    def fill_uniform(self, x, seed: int, offset: int = 0):
        """Device generator of the bench input: x = 2u-1, u = (splitmix64(seed ^ (offset+i)) >> 11) 2^-53."""
        if not _is_device_tensor(x):
            raise TypeError("fill_uniform needs a CUDA tensor")
        self.bind_torch_stream()
        fn = self.lib.vw_fill_uniform_f32 if x.dtype == torch.float32 else self.lib.vw_fill_uniform_f64
        _check(fn(self.ctx, c_void_p(x.data_ptr()), x.numel(), ctypes.c_uint64(seed), offset))
        return x


class Graph:
    """An executable HIP graph of recorded engine calls; ``launch(count)`` replays it on the stream."""

    def __init__(self, engine: Engine, handle: c_void_p, keep=None, result=None):
        self.engine = engine
        self.handle = handle
        self._keep = keep or []   # storage the recorded kernels read / write (see Engine.capture)
        self.result = result

    def launch(self, count: int = 1) -> None:
        _check(self.engine.lib.vw_graph_launch(self.handle, int(count)))

    def stats(self) -> Tuple[int, int]:
        """(kernel nodes, forward -> inverse pairs recorded as one round-trip launch) -- vw_graph_stats."""
        from ctypes import c_int
        k, f = c_int(), c_int()
        _check(self.engine.lib.vw_graph_stats(self.handle, byref(k), byref(f)))
        return k.value, f.value

    def close(self) -> None:
        if self.handle:
            _check(self.engine.lib.vw_graph_destroy(self.handle))
            self.handle = None
        self._keep = []

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def version() -> str:
    return nat.load().vw_version().decode()


def max_levels(N: int, L: int) -> int:
    return int(nat.load().vw_max_levels(N, L))
