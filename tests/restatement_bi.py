"""Numpy restatement of the MODWT loops for banks with TWO filter lengths (test infrastructure, not a test module):
``restatement_generic`` with a low-pass of Llo taps and a high-pass of Lhi taps, as the reference runs
BiorthogonalSpline / ReverseBiorthogonalSpline (paths under vectorwave-core/src/main/java/com/morphiqlabs/wavelet).

  forward            each filter convolved on its own over its own taps, ascending (modwt/MultiLevelMODWTTransform
                     .java:731-754; single level modwt/MODWTTransform.java:131-189)
  inverse PERIODIC   every low tap, then every high tap, one accumulator (:578-588)
  inverse SYMMETRIC  decide() keyed on the LOW length; tauH = tau(Llo, j) + dH, tauG = tau(Lhi, j) + dG (:604-608)
  inverse ZERO, and every single-level inverse: pairwise ``acc += lo[l] * a + hi[l] * d`` over l < Llo_j, reading
                     high[l] -- a longer high-pass is truncated to Llo taps, a shorter one raises IndexError where
                     Java throws ArrayIndexOutOfBoundsException (:591-601, MODWTTransform.java:203-299)
  FFT switch         per filter (WaveletOperations.java:31-33 behind the gate of :734): ``fft_modes`` says which
                     filters of a level take the zero-padded linear convolution over nextPow2(N), and
                     ``fft=True`` in ``decompose`` applies that index map to them.

Arithmetic as restatement_generic: ``acc = acc + x * f`` per tap, product rounded then sum rounded, taps
``dtype(h * (1 / sqrt(2)))``; ``fma=True`` switches every step to the FMA mode's (``accumulate`` /
``accumulate_pair`` of restatement_generic: ``fma(x, f, acc)`` and ``acc + fma(lo, a, round(hi * d))``).  Only the base taps are visited (zero taps of the upsampled filter leave a finite sum
unchanged); ``decompose_full`` / ``reconstruct_full`` visit every upsampled tap, zeros included, in the reference's
order -- the non-finite semantics.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from restatement_generic import _sym_index, accumulate, accumulate_pair, scaled_taps

PERIODIC, SYMMETRIC, ZERO_PADDING = O.PERIODIC, O.SYMMETRIC, O.ZERO_PADDING


def upsampled_length(L: int, j: int) -> int:
    return (L - 1) * (1 << (j - 1)) + 1


def fft_modes(n: int, Llo: int, Lhi: int, j: int):
    """(low takes the FFT branch, high takes it) at level j of a PERIODIC decompose of N = n."""
    llo, lhi = upsampled_length(Llo, j), upsampled_length(Lhi, j)
    if n < 64 or llo > n // 2:   # applyScaledMODWT :734: both direct
        return False, False
    pow2 = n & (n - 1) == 0      # zero-padding to nextPow2(N) == N: the FFT branch is the circular convolution
    return (n >= 1024 and llo > n * (1.0 / 8.0) and not pow2, n >= 1024 and lhi > n * (1.0 / 8.0) and not pow2)


def _conv(cur, f, s, boundary, fft_pad=False, fma=False):
    """One filter over one level input: out[t] = sum_l f[l] * x[index(t - l*s)], ascending l."""
    n = cur.shape[-1]
    t = np.arange(n)
    acc = np.zeros_like(cur)
    npow2 = 1 << (n - 1).bit_length()
    for l in range(len(f)):
        idx = t - l * s
        if boundary == PERIODIC and fft_pad:      # linear convolution of the zero-padded rows, modulo nextPow2(N)
            idx = np.mod(idx, npow2)
            ok = idx < n
            src = cur[..., np.where(ok, idx, 0)]
            acc = accumulate(acc, np.where(ok, src, np.zeros_like(src)), f[l], fma)
        elif boundary == PERIODIC:
            acc = accumulate(acc, cur[..., np.mod(idx, n)], f[l], fma)
        elif boundary == ZERO_PADDING:
            ok = idx >= 0
            acc = accumulate(acc, cur[..., np.where(ok, idx, 0)], f[l], fma, ok)
        else:
            acc = accumulate(acc, cur[..., _sym_index(idx, n)], f[l], fma)
    return acc


def decompose(x, lo, hi, boundary: int, levels: int, dtype=np.float64, fft: bool = False, fma: bool = False):
    """x [N] or [B, N] -> (details [J, (B,) N], approx [(B,) N]); ``lo`` / ``hi`` the ANALYSIS pair."""
    dtype = np.dtype(dtype).type
    cur = np.ascontiguousarray(np.asarray(x), dtype=dtype)
    n = cur.shape[-1]
    if levels < 1 or max(upsampled_length(len(lo), levels), upsampled_length(len(hi), levels)) > n:
        raise ValueError(f"level {levels} filters do not fit N={n}")
    flo, fhi = scaled_taps(lo, dtype), scaled_taps(hi, dtype)
    det = np.empty((levels,) + cur.shape, dtype=dtype)
    for j in range(1, levels + 1):
        s = 1 << (j - 1)
        f_lo, f_hi = fft_modes(n, len(lo), len(hi), j) if (fft and boundary == PERIODIC) else (False, False)
        det[j - 1] = _conv(cur, fhi, s, boundary, f_hi, fma)
        cur = _conv(cur, flo, s, boundary, f_lo, fma)
    return det, cur


def forward1(x, lo, hi, boundary: int, dtype=np.float64, fma: bool = False):
    """MODWTTransform.forward: (approx, detail), any N >= 1."""
    dtype = np.dtype(dtype).type
    cur = np.ascontiguousarray(np.asarray(x), dtype=dtype)
    return (_conv(cur, scaled_taps(lo, dtype), 1, boundary, fma=fma),
            _conv(cur, scaled_taps(hi, dtype), 1, boundary, fma=fma))


def _pairwise(a, d, flo, fhi, s, index, fma=False):
    """acc += lo[l] * a[idx] + hi[l] * d[idx] over l < Llo, reading high[l] (the reference's truncation / throw)."""
    if len(fhi) < len(flo):
        raise IndexError(f"Index {len(fhi)} out of bounds for length {len(fhi)}")  # Java's exception at l = Lhi
    n = a.shape[-1]
    t = np.arange(n)
    acc = np.zeros_like(a)
    for l in range(len(flo)):
        ok, src = index(t, l * s, n)
        acc = accumulate_pair(acc, a[..., src], flo[l], d[..., src], fhi[l], fma, ok)
    return acc


def _idx_zero(t, off, n):
    idx = t + off
    ok = idx < n
    return ok, np.where(ok, idx, 0)


def _inverse_level(a, d, flo, fhi, s, boundary, align, fma=False):
    n = a.shape[-1]
    t = np.arange(n)
    if boundary == ZERO_PADDING:
        return _pairwise(a, d, flo, fhi, s, _idx_zero, fma)
    acc = np.zeros_like(a)
    if boundary == PERIODIC:
        for l in range(len(flo)):
            acc = accumulate(acc, a[..., np.mod(t + l * s, n)], flo[l], fma)
        for l in range(len(fhi)):
            acc = accumulate(acc, d[..., np.mod(t + l * s, n)], fhi[l], fma)
        return acc
    approx_plus, tau_h, detail_plus, tau_g = align
    for l in range(len(flo)):
        idx = t + l * s - tau_h if approx_plus else t - l * s + tau_h
        acc = accumulate(acc, a[..., _sym_index(idx, n)], flo[l], fma)
    for l in range(len(fhi)):
        idx = t + l * s - tau_g if detail_plus else t - l * s + tau_g
        acc = accumulate(acc, d[..., _sym_index(idx, n)], fhi[l], fma)
    return acc


def sym_align(wavelet_id: int, Llo: int, Lhi: int, j: int):
    ap, dh, dp, dg = O.sym_decide(wavelet_id, Llo, j)
    return ap, O.lib().vwo_compute_tau(Llo, j) + dh, dp, O.lib().vwo_compute_tau(Lhi, j) + dg


def reconstruct(det, app, lo, hi, boundary: int, wavelet_id: int = 0, detail_mask: int = 0xFFFFFFFF,
                approx_zero: bool = False, dtype=np.float64, fma: bool = False):
    """det [J, (B,) N], app [(B,) N] -> y; ``lo`` / ``hi`` the SYNTHESIS pair."""
    dtype = np.dtype(dtype).type
    det = np.ascontiguousarray(np.asarray(det), dtype=dtype)
    cur = np.ascontiguousarray(np.asarray(app), dtype=dtype)
    J, n = det.shape[0], cur.shape[-1]
    if max(upsampled_length(len(lo), J), upsampled_length(len(hi), J)) > n:
        raise ValueError(f"level {J} filters do not fit N={n}")
    flo, fhi = scaled_taps(lo, dtype), scaled_taps(hi, dtype)
    if approx_zero:
        cur = np.zeros_like(cur)
    zero = np.zeros_like(cur)
    for j in range(J, 0, -1):
        align = sym_align(wavelet_id, len(lo), len(hi), j) if boundary == SYMMETRIC else None
        d = det[j - 1] if (detail_mask >> (j - 1)) & 1 else zero
        cur = _inverse_level(cur, d, flo, fhi, 1 << (j - 1), boundary, align, fma)
    return cur


def inverse1(approx, detail, lo, hi, boundary: int, batch_sym: bool = False, dtype=np.float64, fma: bool = False):
    """MODWTTransform.inverse: pairwise in all three boundaries; SYMMETRIC reads t - l (``batch_sym``: t + l)."""
    dtype = np.dtype(dtype).type
    a = np.ascontiguousarray(np.asarray(approx), dtype=dtype)
    d = np.ascontiguousarray(np.asarray(detail), dtype=dtype)
    flo, fhi = scaled_taps(lo, dtype), scaled_taps(hi, dtype)
    if boundary == ZERO_PADDING:
        index = _idx_zero
    elif boundary == PERIODIC:
        index = lambda t, off, n: (None, np.mod(t + off, n))
    else:
        index = lambda t, off, n: (None, _sym_index(t + off if batch_sym else t - off, n))
    return _pairwise(a, d, flo, fhi, 1, index, fma)


# ---- every upsampled tap, zeros included (VW_FLAG_REF_NONFINITE): slow scalar-order loops over l ----------------
def _upsample(f, s, dtype):
    out = [dtype(0)] * ((len(f) - 1) * s + 1)
    for i, v in enumerate(f):
        out[i * s] = v
    return out


def decompose_full(x, lo, hi, boundary: int, levels: int, dtype=np.float64):
    dtype = np.dtype(dtype).type
    cur = np.ascontiguousarray(np.asarray(x), dtype=dtype)
    flo, fhi = scaled_taps(lo, dtype), scaled_taps(hi, dtype)
    det = np.empty((levels,) + cur.shape, dtype=dtype)
    with np.errstate(invalid="ignore"):
        for j in range(1, levels + 1):
            s = 1 << (j - 1)
            det[j - 1] = _conv(cur, _upsample(fhi, s, dtype), 1, boundary)
            cur = _conv(cur, _upsample(flo, s, dtype), 1, boundary)
    return det, cur


def reconstruct_full(det, app, lo, hi, boundary: int, wavelet_id: int = 0, dtype=np.float64):
    dtype = np.dtype(dtype).type
    det = np.ascontiguousarray(np.asarray(det), dtype=dtype)
    cur = np.ascontiguousarray(np.asarray(app), dtype=dtype)
    flo, fhi = scaled_taps(lo, dtype), scaled_taps(hi, dtype)
    with np.errstate(invalid="ignore"):
        for j in range(det.shape[0], 0, -1):
            s = 1 << (j - 1)
            align = sym_align(wavelet_id, len(lo), len(hi), j) if boundary == SYMMETRIC else None
            cur = _inverse_level(cur, det[j - 1], _upsample(flo, s, dtype), _upsample(fhi, s, dtype), 1, boundary, align)
    return cur
