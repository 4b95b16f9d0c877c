"""Wavelet energy per level, the parts that need no GPU: the C ABI exports and refuses a null context, the host
path of MultiLevelMODWTResult.energiesPerSignal is the reference's sequential loop, and the relative form follows
MultiLevelMODWTResultImpl.getRelativeEnergyDistribution (:121-138) in order and in its zero-total rule."""
import numpy as np

import energy_restatement as ER
from vectorwave_amd import _native as nat
from vectorwave_amd import errors
from vectorwave_amd.modwt import MultiLevelMODWTResult, relative_energy


def _loop_energy(c) -> float:
    e = 0.0
    for v in c:
        e += float(v) * float(v)
    return e


def test_restatement_is_the_sequential_loop():
    c = np.random.default_rng(7).standard_normal(257) * 1e3
    assert ER.seq_energy(c) == _loop_energy(c)
    assert ER.seq_energy([]) == 0.0


def test_symbols_exported_and_in_signature_table():
    lib = nat.load()
    for name in ("vw_modwt_energy_f64", "vw_energy_planes_f64"):
        assert hasattr(lib, name), name
        assert name in nat.SIGNATURES, name


def test_null_context_maps_to_npe():
    lib = nat.load()
    lo = nat.taps_array([0.5, 0.5])
    out = np.zeros(2)
    st = lib.vw_modwt_energy_f64(None, out.ctypes.data, 1, 4, 4, lo, lo, 2, 0, 0, 1, 0, out.ctypes.data)
    assert st == errors.VW_ERR_NULL and "null" in nat.last_error()
    st = lib.vw_energy_planes_f64(None, out.ctypes.data, out.ctypes.data, 1, 4, 1, 0, out.ctypes.data)
    assert st == errors.VW_ERR_NULL and "null" in nat.last_error()


def test_host_energies_per_signal_equal_the_loop():
    rng = np.random.default_rng(11)
    det, app = rng.standard_normal((3, 4, 129)), rng.standard_normal((4, 129))
    app[2] = 0.0
    got = MultiLevelMODWTResult(det, app).energiesPerSignal()
    assert got.shape == (4, 4)
    for b in range(4):
        assert got[0, b] == _loop_energy(app[b])
        for j in range(3):
            assert got[j + 1, b] == _loop_energy(det[j, b])
    assert got[0, 2] == 0.0 and not np.signbit(got[0, 2])
    assert np.array_equal(got, ER.planes_energies(det, app))
    # a single signal is a batch of one
    one = MultiLevelMODWTResult(det[:, 1], app[1]).energiesPerSignal()
    assert one.shape == (4, 1) and np.array_equal(one[:, 0], got[:, 1])


def test_relative_energy_order_zero_rows_and_accumulation_order():
    # (a + d1) + d2 != a + (d1 + d2) in fp64: the total must be accumulated approx first, then d1, d2
    a, d1, d2 = 1.0, 2.0 ** -53, 2.0 ** -53
    assert (a + d1) + d2 != a + (d1 + d2)
    e = np.array([[a, 0.0, 3.0], [d1, 0.0, 1.0], [d2, 0.0, 4.0]])
    got = relative_energy(e)
    total = (a + d1) + d2
    assert np.array_equal(got[:, 0], [a / total, d1 / total, d2 / total])
    wrong = a + (d1 + d2)
    assert got[0, 0] != a / wrong
    assert np.array_equal(got[:, 1], [0.0, 0.0, 0.0]) and not np.signbit(got[:, 1]).any()
    assert np.array_equal(got[:, 2], [3.0 / 8.0, 1.0 / 8.0, 4.0 / 8.0])   # [approx, d1, d2]
    assert np.array_equal(got, ER.relative(e))
