"""The energy JNI natives (modwtEnergyAoS / energyPlanesAoS in jni/vectorwave_amd_jni.c) through the fake JNIEnv of
tests/jni_harness: each native equals the direct C-ABI call on the same rows, over batches that span several
64 KiB row chunks (one ending exactly on a chunk, one in a partial chunk); null and ragged rows raise; a NaN in a
later chunk names the batch's signal; no local reference survives a call (checked by Jni.call after every native)."""
from ctypes import c_void_p

import numpy as np
import pytest

import energy_restatement as ER
from oracle import oracle as O
from test_jni_glue import IAE, NPE, PFX, Jni, _harness, chunk_rows, ctx_of, i, l, o, taps
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import Daubechies

pytestmark = pytest.mark.gpu

HOST = nat.FLAG_HOST_MEMORY | nat.FLAG_SYNC
NATIVES = {
    "modwtEnergyAoS": (i, [l, o, o, o, i, i, i, i, o]),
    "energyPlanesAoS": (i, [l, o, o, i, o]),
}
W = Daubechies.DB4
N, J = 1001, 3


@pytest.fixture(scope="module")
def jni():
    L = _harness()
    for name, (res, args) in NATIVES.items():
        f = getattr(L, PFX + name)
        f.restype, f.argtypes = res, [o, o] + args
    return Jni(L)


def _signals(B):
    return np.random.default_rng(B).standard_normal((B, N))


def _cabi_energy(engine, x, flags):
    B = x.shape[0]
    out = np.empty((J + 1, B))
    lo, hi = taps(W)
    st = engine.lib.vw_modwt_energy_f64(engine.ctx, c_void_p(x.ctypes.data), B, N, N, nat.taps_array(lo),
                                        nat.taps_array(hi), len(lo), W.wavelet_id, O.PERIODIC, J, flags | HOST,
                                        c_void_p(out.ctypes.data))
    assert st == 0, nat.last_error()
    return out


@pytest.mark.parametrize("B", [40, 43], ids=["whole-chunks", "partial-last-chunk"])
def test_energy_native_matches_the_c_abi(engine, jni, B):
    cb = chunk_rows(N + J + 1, B)
    assert cb == 8 and B > 2 * cb and (B % cb != 0) == (B == 43)
    x = _signals(B)
    lo, hi = taps(W)
    for flags in (nat.FLAG_CORE_LEVELS, nat.FLAG_CORE_LEVELS | nat.FLAG_TREE_SUMS, nat.FLAG_VALIDATE):
        out = np.full((J + 1) * B, -7.0)
        st, pend = jni.call("modwtEnergyAoS", ctx_of(engine), jni.rows(x), jni.doubles(lo), jni.doubles(hi),
                            W.wavelet_id, O.PERIODIC, J, flags, jni.doubles(out))
        assert st == 0 and pend is None
        assert np.array_equal(out.reshape(J + 1, B), _cabi_energy(engine, x, flags))
    assert np.array_equal(out.reshape(J + 1, B), ER.energies(x, lo, hi, O.PERIODIC, J))   # and the restatement


@pytest.mark.parametrize("B", [8, 11], ids=["whole-chunks", "partial-last-chunk"])
def test_planes_native_matches_the_c_abi(engine, jni, B):
    cb = chunk_rows((J + 1) * (N + 1), B)
    assert cb == 2 and B > 2 * cb and (B % cb != 0) == (B == 11)
    rng = np.random.default_rng(200 + B)
    det, app = rng.standard_normal((J, B, N)), rng.standard_normal((B, N))
    for flags in (0, nat.FLAG_TREE_SUMS):
        out, ref = np.full((J + 1) * B, -7.0), np.empty((J + 1, B))
        st, pend = jni.call("energyPlanesAoS", ctx_of(engine), jni.planes(det), jni.rows(app), flags, jni.doubles(out))
        assert st == 0 and pend is None
        assert engine.lib.vw_energy_planes_f64(engine.ctx, c_void_p(det.ctypes.data), c_void_p(app.ctypes.data), B, N,
                                               J, flags | HOST, c_void_p(ref.ctypes.data)) == 0
        assert np.array_equal(out.reshape(J + 1, B), ref)
        if not flags:
            assert np.array_equal(ref, ER.planes_energies(det, app))


def test_malformed_rows_raise(engine, jni):
    x = _signals(12)
    lo, hi = taps(W)
    out = np.zeros((J + 1) * 12)
    rows = list(x)
    null_late = rows[:10] + [None] + rows[11:]      # in the second chunk: the first chunk has run
    ragged = rows[:9] + [rows[9][:500]] + rows[10:]
    args = lambda r: (r, jni.doubles(lo), jni.doubles(hi), W.wavelet_id, O.PERIODIC, J, 0)  # noqa: E731
    st, _ = jni.call("modwtEnergyAoS", ctx_of(engine), *args(jni.rows(null_late)), jni.doubles(out),
                     expect=(IAE, "non-null and same length"))
    assert st == 7
    jni.call("modwtEnergyAoS", ctx_of(engine), *args(jni.rows(ragged)), jni.doubles(out),
             expect=(IAE, "non-null and same length"))
    jni.call("modwtEnergyAoS", ctx_of(engine), *args(None), jni.doubles(out), expect=(IAE, "non-null and non-empty"))
    jni.call("modwtEnergyAoS", ctx_of(engine), *args(jni.rows(x)), jni.doubles(out[:5]), expect=(IAE, "shorter"))
    jni.call("modwtEnergyAoS", ctx_of(engine), *args(jni.rows(x)), None, expect=(NPE, "output"))
    det = np.zeros((J, 12, N))
    jni.call("energyPlanesAoS", ctx_of(engine), None, jni.rows(x), 0, jni.doubles(out), expect=(NPE, "details"))
    jni.call("energyPlanesAoS", ctx_of(engine), jni.planes(det[:, :11]), jni.rows(x), 0, jni.doubles(out),
             expect=(IAE, "length=batch"))
    jni.call("energyPlanesAoS", ctx_of(engine), jni.planes(det), jni.rows(ragged), 0, jni.doubles(out),
             expect=(IAE, "non-null and same length"))


def test_validation_error_names_the_batch_signal(engine, jni):
    B = 40
    x = _signals(B)
    x[21, 77] = np.nan                               # third chunk (rows 16-23)
    lo, hi = taps(W)
    out = np.zeros((J + 1) * B)
    st, pend = jni.call("modwtEnergyAoS", ctx_of(engine), jni.rows(x), jni.doubles(lo), jni.doubles(hi), W.wavelet_id,
                        O.PERIODIC, J, nat.FLAG_VALIDATE, jni.doubles(out))
    assert st == 3 and pend is None
    msg = jni.last_error()
    assert "non-finite" in msg and "signal 21)" in msg and "index 77" in msg, msg
    assert jni.raw("lastErrorIndex") == 77
