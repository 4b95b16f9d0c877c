"""The biorthogonal catalogue (vectorwave_amd.wavelets.BiorthogonalSpline / ReverseBiorthogonalSpline) against the
reference's stored arrays, bit for bit: tests/golden/bior_taps.json holds, per name, lowPassDecomposition and
lowPassReconstruction as hex floats (written by tests/golden/make_bior_fixture.py from the reference's source
text); the high-pass filters follow from them by BiorthogonalSpline.java:309-339's sign rule, restated here."""
import json
import os

import pytest

import vectorwave_amd as vw
from vectorwave_amd.wavelets import WID_OTHER, BiorthogonalWavelet, available_wavelets, get_wavelet, is_biorthogonal

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "bior_taps.json")) as _f:
    TAPS = json.load(_f)

ORDERS = ["1.1", "1.3", "1.5", "2.2", "2.4", "2.6", "2.8", "3.1", "3.3", "3.5", "3.7", "3.9", "4.4", "5.5", "6.8"]
NAMES = ["bior" + o for o in ORDERS] + ["rbio" + o for o in ORDERS]


def _mirror(h):
    """g[i] = sign * h[n-1-i], sign = +1 when (n-1-i) is even (Java: an int sign times a double)."""
    n = len(h)
    return [(1 if (n - 1 - i) % 2 == 0 else -1) * h[n - 1 - i] for i in range(n)]


def _bits(values):
    return [float(v).hex() for v in values]


def test_fixture_lists_the_thirty_names():
    assert sorted(TAPS) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_four_accessors_bit_for_bit(name):
    w = get_wavelet(name)
    dec = [float.fromhex(s) for s in TAPS[name]["dec"]]
    rec = [float.fromhex(s) for s in TAPS[name]["rec"]]
    assert isinstance(w, BiorthogonalWavelet) and w.name() == name
    assert _bits(w.lowPassDecomposition()) == _bits(dec)
    assert _bits(w.lowPassReconstruction()) == _bits(rec)
    assert _bits(w.highPassDecomposition()) == _bits(_mirror(rec))
    assert _bits(w.highPassReconstruction()) == _bits(_mirror(dec))
    assert w.filter_length == len(dec)
    assert w.wavelet_id == WID_OTHER


def test_length_patterns():
    """The analysis pair is (len(dec), len(rec)), the synthesis pair the swap; rbio swaps the sides."""
    want = {"bior1.1": (2, 2), "bior1.3": (6, 2), "bior2.2": (5, 3), "bior4.4": (9, 7), "bior3.9": (20, 4),
            "bior6.8": (17, 16), "rbio1.5": (2, 10), "rbio4.4": (7, 9)}
    for name, (llo, lhi) in want.items():
        w = get_wavelet(name)
        assert (len(w.lowPassDecomposition()), len(w.highPassDecomposition())) == (llo, lhi), name
        assert (len(w.lowPassReconstruction()), len(w.highPassReconstruction())) == (lhi, llo), name


def test_sign_rule_differs_from_the_orthogonal_qmf_at_even_lengths():
    w = get_wavelet("bior1.3")  # reconstruction low-pass {1, 1}: g = {-1, 1}, where (-1)^i would give {1, -1}
    assert w.highPassDecomposition() == [-1.0, 1.0]


def test_class_attributes_and_registry():
    assert vw.BiorthogonalSpline.BIOR4_4 is get_wavelet("bior4.4")
    assert vw.ReverseBiorthogonalSpline.RBIO2_2 is get_wavelet("rbio2.2")
    assert set(NAMES) <= set(available_wavelets())
    r, b = vw.ReverseBiorthogonalSpline.RBIO3_9, vw.BiorthogonalSpline.BIOR3_9
    assert r.lowPassDecomposition() == b.lowPassReconstruction()
    assert r.highPassDecomposition() == b.highPassReconstruction()
    assert r.lowPassReconstruction() == b.lowPassDecomposition()
    assert r.highPassReconstruction() == b.highPassDecomposition()


def test_is_biorthogonal():
    assert not is_biorthogonal(vw.Daubechies.DB4) and not is_biorthogonal(vw.Haar.INSTANCE)
    assert is_biorthogonal(get_wavelet("bior4.4")) and is_biorthogonal(get_wavelet("rbio1.5"))
    # bior1.1 stores Haar's low-pass on both sides: its decomposition and reconstruction filters are equal, so the
    # paths that take one filter pair may run it
    assert not is_biorthogonal(get_wavelet("bior1.1"))
