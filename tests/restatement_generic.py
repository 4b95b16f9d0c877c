"""Dtype-generic numpy restatement of the multi-level decompose / reconstruct (test infrastructure, not a test
module).

The loops are those of ``oracle/vw_oracle.c`` (vwo_ml_decompose, apply_scaled_inverse, vwo_ml_reconstruct), written
as one array operation per tap: every output is one running sum ``acc = acc + x * f`` -- product rounded, then the
sum rounded -- tap by tap in ascending tap order, the low-pass branch before the high-pass branch, and the
ZERO_PADDING inverse as ``acc += lo * a + hi * d``.  Only the L taps of the base filter are visited: the zero taps
of the upsampled filter add +-0 to a finite sum and leave it unchanged.

``fma=True`` restates the engine's FMA mode (VW_FLAG_FMA; madd<FMA> / pair_term<FMA> in vw_dev_core.h) with the
same indexing: the running sum becomes ``acc = fma(x, f, acc)``, ONE rounding per tap, and the pairwise term
``acc + fma(lo, a, round(hi * d))`` -- the high-pass product rounded, the low-pass product fused into it, the sum
with the accumulator rounded.  The fused step is libm's fma / fmaf through the oracle library (``O.fma_f64`` /
``O.fma_f32``), correctly rounded in the element type.  Both accumulate forms live in ``accumulate`` and
``accumulate_pair``, the only places a mode is looked at, so a restatement cannot mix modes.

ZERO_PADDING in FMA mode visits every base tap with +0 for a sample outside the row, as the kernels do (their halo
holds zeros).  In EXACT mode skipping those taps is exact -- ``acc + round(x * f)`` never leaves -0 in a sum that
started at +0 -- but a fused chain whose only terms so far underflowed completely (float32: |x * f| < 2**-150) holds
-0, and a later ``fma(+0, f, -0)`` with f > 0 turns it back into +0.  The sign of such a zero is all that differs.

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


def accumulate(acc, x, f, fma=False, ok=None):
    """The running sum's step.  EXACT: ``acc + x * f``, product rounded then sum rounded.  FMA: ``fma(x, f, acc)``,
    one rounding, in the arrays' element type.  ``ok`` (ZERO_PADDING): which samples lie inside the row -- EXACT
    skips the others, FMA takes them as +0 (see the module docstring)."""
    if fma:
        if ok is not None:
            x = np.where(ok, x, np.zeros_like(x))
        return (O.fma_f32 if acc.dtype == np.float32 else O.fma_f64)(x, f, acc)
    nxt = acc + x * f
    return nxt if ok is None else np.where(ok, nxt, acc)


def accumulate_pair(acc, a, lo, d, hi, fma=False, ok=None):
    """The pairwise inverse's step.  EXACT: ``acc + (lo * a + hi * d)``.  FMA: ``acc + fma(lo, a, round(hi * d))``
    (pair_term<FMA>: the high-pass product rounded, the low-pass product fused, then a rounded add).  ``ok``: samples
    outside the row are skipped in both modes (the rounded add of a +-0 term cannot change a sum that is never -0)."""
    if fma:
        nxt = acc + (O.fma_f32 if acc.dtype == np.float32 else O.fma_f64)(a, lo, hi * d)
    else:
        nxt = acc + (lo * a + hi * d)
    return nxt if ok is None else np.where(ok, nxt, acc)


def _sym_index(idx, n):
    """MathUtils.symmetricBoundaryExtension (vwo_symmetric_index), vectorised."""
    m = np.mod(idx, 2 * n)
    return np.where(m >= n, 2 * n - m - 1, m)


def _forward_level(cur, flo, fhi, s, boundary, fma=False):
    n = cur.shape[-1]
    t = np.arange(n)
    a = np.zeros_like(cur)
    d = np.zeros_like(cur)
    for l in range(len(flo)):
        idx = t - l * s
        if boundary == PERIODIC:
            src = cur[..., np.mod(idx, n)]
            a = accumulate(a, src, flo[l], fma)
            d = accumulate(d, src, fhi[l], fma)
        elif boundary == ZERO_PADDING:
            ok = idx >= 0
            src = cur[..., np.where(ok, idx, 0)]
            a = accumulate(a, src, flo[l], fma, ok)
            d = accumulate(d, src, fhi[l], fma, ok)
        else:
            src = cur[..., _sym_index(idx, n)]
            a = accumulate(a, src, flo[l], fma)
            d = accumulate(d, src, fhi[l], fma)
    return a, d


def decompose(x, lo, hi, boundary: int, levels: int, dtype=np.float64, fma: bool = False):
    """x [N] or [B, N] -> (details [J, (B,) N], approx [(B,) N]) in ``dtype``; ``fma``: the FMA mode's sums."""
    dtype = np.dtype(dtype).type
    cur = np.ascontiguousarray(np.asarray(x), dtype=dtype)
    n = cur.shape[-1]
    L = len(lo)
    if levels < 1 or (L - 1) * (1 << (levels - 1)) + 1 > n:
        raise ValueError(f"level {levels} filter does not fit N={n}")
    flo, fhi = scaled_taps(lo, dtype), scaled_taps(hi, dtype)
    det = np.empty((levels,) + cur.shape, dtype=dtype)
    for j in range(1, levels + 1):
        cur, det[j - 1] = _forward_level(cur, flo, fhi, 1 << (j - 1), boundary, fma)
    return det, cur


def _inverse_level(a, d, flo, fhi, s, boundary, align, fma=False):
    n = a.shape[-1]
    t = np.arange(n)
    acc = np.zeros_like(a)
    L = len(flo)
    if boundary == PERIODIC:
        for l in range(L):
            acc = accumulate(acc, a[..., np.mod(t + l * s, n)], flo[l], fma)
        for l in range(L):
            acc = accumulate(acc, d[..., np.mod(t + l * s, n)], fhi[l], fma)
    elif boundary == ZERO_PADDING:
        for l in range(L):
            idx = t + l * s
            ok = idx < n
            src = np.where(ok, idx, 0)
            acc = accumulate_pair(acc, a[..., src], flo[l], d[..., src], fhi[l], fma, ok)
    else:
        approx_plus, tau_h, detail_plus, tau_g = align
        for l in range(L):
            idx = t + l * s - tau_h if approx_plus else t - l * s + tau_h
            acc = accumulate(acc, a[..., _sym_index(idx, n)], flo[l], fma)
        for l in range(L):
            idx = t + l * s - tau_g if detail_plus else t - l * s + tau_g
            acc = accumulate(acc, d[..., _sym_index(idx, n)], fhi[l], fma)
    return acc


def reconstruct(det, app, lo, hi, boundary: int, wavelet_id: int = 0, detail_mask: int = 0xFFFFFFFF,
                approx_zero: bool = False, dtype=np.float64, fma: bool = False):
    """det [J, (B,) N], app [(B,) N] -> y [(B,) N] in ``dtype`` (cascade J..1; a cleared ``detail_mask`` bit j-1
    runs level j on zero details, ``approx_zero`` starts from zeros; ``fma``: the FMA mode's sums)."""
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
        cur = _inverse_level(cur, d, flo, fhi, 1 << (j - 1), boundary, align, fma)
    return cur
