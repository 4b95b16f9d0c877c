"""tests/restatement_generic.py at float64 against the C restatement (oracle/vw_oracle.c), bit for bit: the numpy
loops, one array operation per tap, are the oracle's sums in the oracle's order.  That is what entitles the same
code at float32 to serve as the bit-level reference of the fp32 kernels (tests/test_gpu_f32_parity.py)."""
import numpy as np
import pytest

from oracle import oracle as O
from vectorwave_amd.wavelets import WID_OTHER, Coiflet, Daubechies, Haar, Symlet

import restatement_generic as G

SYN28 = G.synthetic_filter(28)
FILTERS = {
    "haar": (Haar.INSTANCE.lowPassDecomposition(), Haar.INSTANCE.highPassDecomposition(), Haar.INSTANCE.wavelet_id),
    "db4": (Daubechies.DB4.lowPassDecomposition(), Daubechies.DB4.highPassDecomposition(), Daubechies.DB4.wavelet_id),
    "sym8": (Symlet.SYM8.lowPassDecomposition(), Symlet.SYM8.highPassDecomposition(), Symlet.SYM8.wavelet_id),
    "coif5": (Coiflet.COIF5.lowPassDecomposition(), Coiflet.COIF5.highPassDecomposition(), Coiflet.COIF5.wavelet_id),
    "syn28": (SYN28[0], SYN28[1], WID_OTHER),
}
BOUNDARIES = [O.PERIODIC, O.SYMMETRIC, O.ZERO_PADDING]


def exact(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    if not np.array_equal(a, b):
        i = np.unravel_index(np.argmax(np.abs(a - b)), a.shape)
        raise AssertionError(f"not bit-exact: max |diff| = {np.max(np.abs(a - b)):.3e} at {i}")


@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=["P", "S", "Z"])
@pytest.mark.parametrize("n", [64, 129, 1000])
def test_float64_equals_the_oracle(name, boundary, n):
    lo, hi, wid = FILTERS[name]
    L = len(lo)
    J = min(4, O.max_levels(n, L))
    assert J >= 1
    x = np.stack([O.java_random_signal(n, 7 + b) for b in range(2)])
    det, app = G.decompose(x, lo, hi, boundary, J)
    assert det.shape == (J, 2, n) and app.shape == (2, n)
    masks = [((1 << J) - 1, False), (0b110 & ((1 << J) - 1), False), (0b001, True), (0b110 & ((1 << J) - 1), True)]
    for b in range(2):
        # every n < 1024: the core decompose never enters its FFT region
        d_ref, a_ref = O.decompose(x[b], lo, hi, boundary, J)
        exact(det[:, b, :], d_ref)
        exact(app[b], a_ref)
        if boundary == O.PERIODIC:  # the batch facade's loop, (t - l + N) % N over every upsampled tap: the same sums
            d_b, a_b = O.decompose(x[b], lo, hi, boundary, J, core=False)
            exact(det[:, b, :], d_b)
            exact(app[b], a_b)
        for mask, az in masks:
            y_ref = O.reconstruct(d_ref, a_ref, lo, hi, boundary, wid, detail_mask=mask, approx_zero=az)
            exact(G.reconstruct(d_ref, a_ref, lo, hi, boundary, wid, detail_mask=mask, approx_zero=az), y_ref)
    # the batched call is the per-row call
    y = G.reconstruct(det, app, lo, hi, boundary, wid)
    exact(y[1], G.reconstruct(det[:, 1, :], app[1], lo, hi, boundary, wid))


def test_float32_rounds_once_per_operation():
    """The float32 form keeps every intermediate in float32 (no hidden binary64 accumulation): a two-tap sum
    computed by hand with explicit float32 roundings."""
    lo, hi = [0.3, 0.7], [0.7, -0.3]
    x = O.java_random_signal(16, 3)
    det, app = G.decompose(x, lo, hi, O.PERIODIC, 1, dtype=np.float32)
    assert det.dtype == np.float32 and app.dtype == np.float32
    f = G.scaled_taps(lo, np.float32)
    assert f[0] == np.float32(0.3 * (1.0 / np.sqrt(2.0)))
    xs = x.astype(np.float32)
    for t in range(16):
        want = np.float32(np.float32(xs[t] * f[0]) + np.float32(xs[(t - 1) % 16] * f[1]))
        assert app[t] == want


def test_level_that_does_not_fit_raises():
    lo, hi = SYN28
    with pytest.raises(ValueError):
        G.decompose(np.zeros(64), lo, hi, O.PERIODIC, 3)
