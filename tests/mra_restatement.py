"""Skip-zero numpy restatement of the multiresolution analysis (test infrastructure, not a test module).

Component c of a decomposition (details [J], approx) is DEFINED as ``restatement_generic.reconstruct`` with
``detail_mask = 1 << (c-1)`` / ``approx_zero = True`` for c >= 1 and ``detail_mask = 0`` / ``approx_zero = False``
for c = 0 (VectorWaveSwtAdapter.extractLevel).  That cascade runs both branches at every level, on zero arrays
where a plane is masked out.  This module states the form the fused kernel computes: only the branch passes whose
input is not a zeroed plane,

    component 0      low-pass passes at levels J .. 1 on approx
    component c > 0  one high-pass pass at level c on d_c, then low-pass passes at levels c-1 .. 1

each pass ``acc = 0; acc = acc + f[l] * src[index_l(t)]`` in ascending tap order (``fma=True``: the FMA mode's
``acc = fma(src, f[l], acc)``, restatement_generic.accumulate -- k_mra's sums; see ``mra_by_masks`` for the loop
path's).  Every accumulator starts at +0.0
and a sum of finite terms that started at +0.0 is never -0.0, so the skipped ``acc + f * (+-0)`` steps -- and the
zero partner of the ZERO_PADDING pairwise term ``lo * a + hi * 0`` -- could not have changed a bit
(tests/test_mra_restatement_cpu.py compares the two forms byte for byte, signed zeros included).
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from restatement_generic import PERIODIC, SYMMETRIC, ZERO_PADDING, _sym_index, accumulate, reconstruct, scaled_taps


def _branch_pass(src, f, s, boundary, plus, tau, fma=False):
    """One branch of one level: periodic / zero padding read t + l*s; symmetric reads t + l*s - tau (plus) or
    t - l*s + tau through the mirror."""
    n = src.shape[-1]
    t = np.arange(n)
    acc = np.zeros_like(src)
    for l in range(len(f)):
        if boundary == PERIODIC:
            acc = accumulate(acc, src[..., np.mod(t + l * s, n)], f[l], fma)
        elif boundary == ZERO_PADDING:
            idx = t + l * s
            ok = idx < n
            acc = accumulate(acc, src[..., np.where(ok, idx, 0)], f[l], fma, ok)
        else:
            idx = t + l * s - tau if plus else t - l * s + tau
            acc = accumulate(acc, src[..., _sym_index(idx, n)], f[l], fma)
    return acc


def _align(boundary, wavelet_id, L, j):
    """(approx_plus, tau_h, detail_plus, tau_g) of level j, as restatement_generic.reconstruct."""
    if boundary != SYMMETRIC:
        return 1, 0, 1, 0
    ap, dh, dp, dg = O.sym_decide(wavelet_id, L, j)
    tau = O.lib().vwo_compute_tau(L, j)
    return ap, tau + dh, dp, tau + dg


def component(det, app, lo, hi, boundary: int, c: int, wavelet_id: int = 0, dtype=np.float64, fma: bool = False):
    """Component c (0 = smooth, j = detail level j) of det [J, (B,) N] / app [(B,) N], in ``dtype``."""
    dtype = np.dtype(dtype).type
    det = np.ascontiguousarray(np.asarray(det), dtype=dtype)
    app = np.ascontiguousarray(np.asarray(app), dtype=dtype)
    J, n, L = det.shape[0], app.shape[-1], len(lo)
    if not 0 <= c <= J:
        raise ValueError(f"component {c} of a {J}-level decomposition")
    if (L - 1) * (1 << (J - 1)) + 1 > n:
        raise ValueError(f"level {J} filter does not fit N={n}")
    flo, fhi = scaled_taps(lo, dtype), scaled_taps(hi, dtype)
    if c == 0:
        cur, top = app, J
    else:
        ap, th, dp, tg = _align(boundary, wavelet_id, L, c)
        cur, top = _branch_pass(det[c - 1], fhi, 1 << (c - 1), boundary, dp, tg, fma), c - 1
    for j in range(top, 0, -1):
        ap, th, dp, tg = _align(boundary, wavelet_id, L, j)
        cur = _branch_pass(cur, flo, 1 << (j - 1), boundary, ap, th, fma)
    return cur


def mra(det, app, lo, hi, boundary: int, wavelet_id: int = 0, dtype=np.float64, fma: bool = False):
    """All J+1 components, [J+1, (B,) N]: row 0 the smooth, row j detail component j."""
    J = np.asarray(det).shape[0]
    return np.stack([component(det, app, lo, hi, boundary, c, wavelet_id, dtype, fma) for c in range(J + 1)])


def mra_by_masks(det, app, lo, hi, boundary: int, wavelet_id: int = 0, dtype=np.float64, fma: bool = False):
    """The definition: J+1 masked reconstructions (restatement_generic.reconstruct) -- also the sequence of the
    engine's LOOP PATH (J+1 masked inverses).  In FMA mode it equals ``mra`` for PERIODIC and SYMMETRIC
    (``fma(+-0, f, acc) == acc``); for ZERO_PADDING it does not: the masked pairwise term
    ``acc + fma(lo, a, round(hi * 0))`` rounds the product before the add, where the fused kernel's branch pass is
    ``fma(a, lo, acc)``."""
    J = np.asarray(det).shape[0]
    return np.stack([reconstruct(det, app, lo, hi, boundary, wavelet_id, (1 << (c - 1)) if c else 0, c != 0, dtype, fma)
                     for c in range(J + 1)])
