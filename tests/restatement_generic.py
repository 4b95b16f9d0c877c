"""Dtype-generic numpy restatement of the multi-level decompose / reconstruct (test infrastructure, not a test
module).

The loops are those of ``oracle/vw_oracle.c`` (vwo_ml_decompose, apply_scaled_inverse, vwo_ml_reconstruct), written
as one array operation per tap: every output is one running sum ``acc = acc + x * f`` -- product rounded, then the
sum rounded -- tap by tap in ascending tap order, the low-pass branch before the high-pass branch, and the
ZERO_PADDING inverse as ``acc += lo * a + hi * d``.  Only the L taps of the base filter are visited: the zero taps
of the upsampled filter add +-0 to a finite sum and leave it unchanged.

Taps are ``dtype(h * (1 / sqrt(2)))``: scaled in binary64, rounded to the element type once, as the engine's
``copy_taps``.  At ``float64`` the module equals ``oracle.decompose`` / ``oracle.reconstruct`` bit for bit
(tests/test_restatement_generic_cpu.py), which is what entitles the same code at ``float32`` to stand as the
restatement of the fp32 kernels (EXACT mode: no contraction, one rounding per multiply and per add).

The SYMMETRIC inverse alignment (branch direction and shift per level) is integer bookkeeping and comes from the
oracle: ``sym_decide`` and ``vwo_compute_tau``.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as O

PERIODIC, SYMMETRIC, ZERO_PADDING = O.PERIODIC, O.SYMMETRIC, O.ZERO_PADDING


def synthetic_filter(L: int, seed: int = 1000):
    """(lo, hi) of a synthetic L-tap bank for lengths the wavelet catalogue does not have: pseudo-random taps scaled
    to sum(|lo|) == sqrt(2) (each level's gain is then at most 1, as for a real wavelet) and the QMF high-pass
    hi[l] = (-1)**l * lo[L-1-l].  Not orthogonal; the kernels do not care."""
    lo = O.java_random_signal(L, seed + L)
    lo = lo * (math.sqrt(2.0) / float(np.sum(np.abs(lo))))
    hi = np.array([(1 if l % 2 == 0 else -1) * lo[L - 1 - l] for l in range(L)])
    return [float(v) for v in lo], [float(v) for v in hi]


def scaled_taps(h, dtype):
    s = 1.0 / math.sqrt(2.0)
    return [dtype(float(v) * s) for v in h]


def _sym_index(idx, n):
    """MathUtils.symmetricBoundaryExtension (vwo_symmetric_index), vectorised."""
    m = np.mod(idx, 2 * n)
    return np.where(m >= n, 2 * n - m - 1, m)


def _forward_level(cur, flo, fhi, s, boundary):
    n = cur.shape[-1]
    t = np.arange(n)
    a = np.zeros_like(cur)
    d = np.zeros_like(cur)
    for l in range(len(flo)):
        idx = t - l * s
        if boundary == PERIODIC:
            src = cur[..., np.mod(idx, n)]
            a = a + src * flo[l]
            d = d + src * fhi[l]
        elif boundary == ZERO_PADDING:
            ok = idx >= 0
            src = cur[..., np.where(ok, idx, 0)]
            a = np.where(ok, a + src * flo[l], a)
            d = np.where(ok, d + src * fhi[l], d)
        else:
            src = cur[..., _sym_index(idx, n)]
            a = a + src * flo[l]
            d = d + src * fhi[l]
    return a, d


def decompose(x, lo, hi, boundary: int, levels: int, dtype=np.float64):
    """x [N] or [B, N] -> (details [J, (B,) N], approx [(B,) N]) in ``dtype``."""
    dtype = np.dtype(dtype).type
    cur = np.ascontiguousarray(np.asarray(x), dtype=dtype)
    n = cur.shape[-1]
    L = len(lo)
    if levels < 1 or (L - 1) * (1 << (levels - 1)) + 1 > n:
        raise ValueError(f"level {levels} filter does not fit N={n}")
    flo, fhi = scaled_taps(lo, dtype), scaled_taps(hi, dtype)
    det = np.empty((levels,) + cur.shape, dtype=dtype)
    for j in range(1, levels + 1):
        cur, det[j - 1] = _forward_level(cur, flo, fhi, 1 << (j - 1), boundary)
    return det, cur


def _inverse_level(a, d, flo, fhi, s, boundary, align):
    n = a.shape[-1]
    t = np.arange(n)
    acc = np.zeros_like(a)
    L = len(flo)
    if boundary == PERIODIC:
        for l in range(L):
            acc = acc + flo[l] * a[..., np.mod(t + l * s, n)]
        for l in range(L):
            acc = acc + fhi[l] * d[..., np.mod(t + l * s, n)]
    elif boundary == ZERO_PADDING:
        for l in range(L):
            idx = t + l * s
            ok = idx < n
            src = np.where(ok, idx, 0)
            acc = np.where(ok, acc + (flo[l] * a[..., src] + fhi[l] * d[..., src]), acc)
    else:
        approx_plus, tau_h, detail_plus, tau_g = align
        for l in range(L):
            idx = t + l * s - tau_h if approx_plus else t - l * s + tau_h
            acc = acc + flo[l] * a[..., _sym_index(idx, n)]
        for l in range(L):
            idx = t + l * s - tau_g if detail_plus else t - l * s + tau_g
            acc = acc + fhi[l] * d[..., _sym_index(idx, n)]
    return acc


def reconstruct(det, app, lo, hi, boundary: int, wavelet_id: int = 0, detail_mask: int = 0xFFFFFFFF,
                approx_zero: bool = False, dtype=np.float64):
    """det [J, (B,) N], app [(B,) N] -> y [(B,) N] in ``dtype`` (cascade J..1; a cleared ``detail_mask`` bit j-1
    runs level j on zero details, ``approx_zero`` starts from zeros)."""
    dtype = np.dtype(dtype).type
    det = np.ascontiguousarray(np.asarray(det), dtype=dtype)
    cur = np.ascontiguousarray(np.asarray(app), dtype=dtype)
    J, n, L = det.shape[0], cur.shape[-1], len(lo)
    if (L - 1) * (1 << (J - 1)) + 1 > n:
        raise ValueError(f"level {J} filter does not fit N={n}")
    flo, fhi = scaled_taps(lo, dtype), scaled_taps(hi, dtype)
    if approx_zero:
        cur = np.zeros_like(cur)
    zero = np.zeros_like(cur)
    for j in range(J, 0, -1):
        align = None
        if boundary == SYMMETRIC:
            ap, dh, dp, dg = O.sym_decide(wavelet_id, L, j)
            tau = O.lib().vwo_compute_tau(L, j)
            align = (ap, tau + dh, dp, tau + dg)
        d = det[j - 1] if (detail_mask >> (j - 1)) & 1 else zero
        cur = _inverse_level(cur, d, flo, fhi, 1 << (j - 1), boundary, align)
    return cur
