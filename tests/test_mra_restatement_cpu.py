"""tests/mra_restatement.py (the skip-zero form the fused multiresolution kernel computes) against the definition --
J+1 masked reconstructions, every branch run, zero planes included -- byte for byte, signed zeros included; at
float64 also against the C restatement (oracle.reconstruct).  This is what entitles the skip-zero form to be the
bit-level reference of k_mra in tests/test_gpu_mra.py."""
import numpy as np
import pytest

from oracle import oracle as O
from vectorwave_amd.wavelets import WID_OTHER, Coiflet, Daubechies, Haar, Symlet

import mra_restatement as M
import restatement_generic as G


def _bank(w):
    return w.lowPassReconstruction(), w.highPassReconstruction(), w.wavelet_id


FILTERS = {
    "haar": _bank(Haar.INSTANCE),
    "db4": _bank(Daubechies.DB4),
    "sym8": _bank(Symlet.SYM8),
    "coif5": _bank(Coiflet.COIF5),
    "syn9": G.synthetic_filter(9) + (WID_OTHER,),
    "syn22": G.synthetic_filter(22) + (WID_OTHER,),
}
BOUNDARIES = [O.PERIODIC, O.SYMMETRIC, O.ZERO_PADDING]


def rows(n):
    """Signals whose coefficients hold what could expose a skipped +-0 step: a generic row, a coarsely quantised one
    (many exact cancellations), a single spike (mostly exact zeros, of both signs after the filters) and zeros."""
    x = np.zeros((4, n))
    x[0] = O.java_random_signal(n, 11)
    x[1] = np.round(O.java_random_signal(n, 12) * 8.0) / 8.0
    x[2, n // 3] = -1.0
    return x


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    ua, ub = a.view(np.uint8), b.view(np.uint8)
    if not np.array_equal(ua, ub):
        bad = np.argwhere(a.view(f"u{a.itemsize}") != b.view(f"u{b.itemsize}"))
        raise AssertionError(f"{len(bad)} elements differ, first at {tuple(bad[0])}: {a[tuple(bad[0])]!r} vs "
                             f"{b[tuple(bad[0])]!r}")


def fits(L, J, n):
    return (L - 1) * (1 << (J - 1)) + 1 <= n


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=["P", "S", "Z"])
@pytest.mark.parametrize("name", list(FILTERS))
def test_skip_zero_form_equals_masked_reconstructions(name, boundary, dtype):
    lo, hi, wid = FILTERS[name]
    L = len(lo)
    ran = 0
    for n in (64, 61, 256):
        x = rows(n)
        for J in (2, 3, 4):
            if not fits(L, J, n):
                continue
            det, app = G.decompose(x, lo, hi, boundary, J, dtype=dtype)
            got = M.mra(det, app, lo, hi, boundary, wid, dtype=dtype)
            assert got.shape == (J + 1,) + x.shape and got.dtype == np.dtype(dtype)
            same_bytes(got, M.mra_by_masks(det, app, lo, hi, boundary, wid, dtype=dtype))
            if dtype is np.float64:
                for b in (0, 2):
                    for c in range(J + 1):
                        ref = O.reconstruct(det[:, b, :], app[b], lo, hi, boundary, wid,
                                            detail_mask=(1 << (c - 1)) if c else 0, approx_zero=c != 0)
                        same_bytes(got[c, b], ref)
            ran += 1
    assert ran >= 1, "no (N, J) of the sweep fits this filter"


def test_components_add_up_to_the_signal():
    """The additive split: the inverse is linear in its planes, so the components add up to the full reconstruction
    up to rounding -- (J+1) components x J levels x 2 L rounded operations on values of magnitude <= 2, about
    5 * 4 * 16 * 2^-53 * 2 < 1e-13 here (db4, J = 4, PERIODIC); 1e-12 leaves a decade.  (The reconstruction itself
    differs from the signal by the catalogue taps' own precision, about 1e-11.)"""
    lo, hi, wid = FILTERS["db4"]
    x = rows(256)
    det, app = G.decompose(x, Daubechies.DB4.lowPassDecomposition(), Daubechies.DB4.highPassDecomposition(),
                           O.PERIODIC, 4)
    parts = M.mra(det, app, lo, hi, O.PERIODIC, wid)
    assert np.max(np.abs(parts.sum(axis=0) - G.reconstruct(det, app, lo, hi, O.PERIODIC, wid))) < 1e-12


def test_component_out_of_range_raises():
    lo, hi, wid = FILTERS["haar"]
    with pytest.raises(ValueError):
        M.component(np.zeros((2, 16)), np.zeros(16), lo, hi, O.PERIODIC, 3)
