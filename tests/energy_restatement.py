"""Restatement of the wavelet energies (test infrastructure, not a test module).

computeEnergy (core/modwt/MultiLevelMODWTResultImpl.java:211-216) is ``energy = 0.0; for c: energy += c * c``:
each square rounded, then added to the running sum, in index order.  ``np.add.accumulate(c * c)[-1]`` is that
loop (numpy's accumulate is sequential; ``np.sum`` would add pairwise).  The coefficients are the oracle's
(``oracle.decompose``, the C restatement of vectorwave-core's loops).
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O


def seq_energy(c) -> float:
    c = np.asarray(c, dtype=np.float64).ravel()
    if c.size == 0:
        return 0.0
    return float(np.add.accumulate(c * c)[-1])


def planes_energies(details, approx) -> np.ndarray:
    """details [J, B, N], approx [B, N] -> [J+1, B] in [approx, d1..dJ] order."""
    details, approx = np.asarray(details, dtype=np.float64), np.asarray(approx, dtype=np.float64)
    planes = np.concatenate([approx[None], details], axis=0) if details.shape[0] else approx[None]
    return np.add.accumulate(planes * planes, axis=-1)[..., -1]


def energies(x, lo, hi, boundary: int, levels: int, core: bool = True) -> np.ndarray:
    """x [B, N] -> [J+1, B]: ``oracle.decompose`` per row, then the sequential energy of every plane."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty((levels + 1, x.shape[0]))
    for b in range(x.shape[0]):
        det, app = O.decompose(x[b], lo, hi, boundary, levels, core=core)
        out[0, b] = seq_energy(app)
        for j in range(levels):
            out[j + 1, b] = seq_energy(det[j])
    return out


def relative(e) -> np.ndarray:
    """getRelativeEnergyDistribution (:121-138) per column of e [J+1, B], as plain Python loops."""
    e = np.asarray(e, dtype=np.float64)
    out = np.zeros_like(e)
    for b in range(e.shape[1]):
        total = float(e[0, b])
        for j in range(1, e.shape[0]):
            total += float(e[j, b])
        if total == 0.0:
            continue
        for j in range(e.shape[0]):
            out[j, b] = float(e[j, b]) / total
    return out
