"""The multiresolution JNI natives (mraAoS / mraPlanesAoS in jni/vectorwave_amd_jni.c) through the fake JNIEnv of
tests/jni_harness: each native equals the direct C-ABI call on the same rows, over batches that span several
64 KiB row chunks (one ending exactly on a chunk, one in a partial chunk); null and ragged rows raise; a NaN in a
later chunk names the batch's signal; no local reference survives a call (checked by Jni.call after every native)."""
from ctypes import c_void_p

import numpy as np
import pytest

from oracle import oracle as O
from test_jni_glue import IAE, NPE, PFX, Jni, _harness, chunk_rows, ctx_of, i, l, o, taps
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import Daubechies

pytestmark = pytest.mark.gpu

HOST = nat.FLAG_HOST_MEMORY | nat.FLAG_SYNC
NATIVES = {
    "mraAoS": (i, [l, o, o, o, i, i, i, i, o]),
    "mraPlanesAoS": (i, [l, o, o, o, o, i, i, i, o]),
}
W = Daubechies.DB4
N, J = 200, 3


@pytest.fixture(scope="module")
def jni():
    L = _harness()
    for name, (res, args) in NATIVES.items():
        f = getattr(L, PFX + name)
        f.restype, f.argtypes = res, [o, o] + args
    return Jni(L)


def _signals(B):
    return np.random.default_rng(B).uniform(-1, 1, (B, N))


def _cabi_signal(engine, x, boundary, flags):
    B = x.shape[0]
    out = np.empty((J + 1, B, N))
    lo, hi = taps(W)
    st = engine.lib.vw_modwt_mra_f64(engine.ctx, c_void_p(x.ctypes.data), B, N, N, nat.taps_array(lo),
                                     nat.taps_array(hi), len(lo), W.wavelet_id, boundary, J, flags | HOST,
                                     c_void_p(out.ctypes.data))
    assert st == 0, nat.last_error()
    return out


@pytest.mark.parametrize("boundary", [O.PERIODIC, O.SYMMETRIC], ids=["P", "S"])
@pytest.mark.parametrize("B", [24, 27], ids=["whole-chunks", "partial-last-chunk"])
def test_signal_native_matches_the_c_abi(engine, jni, B, boundary):
    cb = chunk_rows((J + 2) * N, B)
    assert cb == 8 and B > 2 * cb and (B % cb != 0) == (B == 27)
    x = _signals(B)
    lo, hi = taps(W)
    for flags in (0, nat.FLAG_CORE_LEVELS | nat.FLAG_FFT_SWITCH, nat.FLAG_VALIDATE | nat.FLAG_REF_NONFINITE, nat.FLAG_FMA):
        out = np.full((J + 1) * B * N, -7.0)
        st, pend = jni.call("mraAoS", ctx_of(engine), jni.rows(x), jni.doubles(lo), jni.doubles(hi), W.wavelet_id,
                            boundary, J, flags, jni.doubles(out))
        assert st == 0 and pend is None
        assert np.array_equal(out.reshape(J + 1, B, N), _cabi_signal(engine, x, boundary, flags))
    if boundary == O.PERIODIC:   # the components add up to the signal (round-trip bar of the inverse tests)
        assert np.max(np.abs(_cabi_signal(engine, x, boundary, 0).sum(axis=0) - x)) < 1e-9


@pytest.mark.parametrize("B", [15, 17], ids=["whole-chunks", "partial-last-chunk"])
def test_planes_native_matches_the_c_abi(engine, jni, B):
    cb = chunk_rows((2 * J + 2) * N, B)
    assert cb == 5 and B > 2 * cb and (B % cb != 0) == (B == 17)
    rng = np.random.default_rng(200 + B)
    det, app = rng.uniform(-1, 1, (J, B, N)), rng.uniform(-1, 1, (B, N))
    lo, hi = taps(W)
    for boundary in (O.PERIODIC, O.SYMMETRIC, O.ZERO_PADDING):
        for flags in (0, nat.FLAG_REF_NONFINITE | nat.FLAG_CORE_LEVELS):
            out, ref = np.full((J + 1) * B * N, -7.0), np.empty((J + 1, B, N))
            st, pend = jni.call("mraPlanesAoS", ctx_of(engine), jni.planes(det), jni.rows(app), jni.doubles(lo),
                                jni.doubles(hi), W.wavelet_id, boundary, flags, jni.doubles(out))
            assert st == 0 and pend is None
            assert engine.lib.vw_mra_planes_f64(engine.ctx, c_void_p(det.ctypes.data), c_void_p(app.ctypes.data), B, N,
                                                nat.taps_array(lo), nat.taps_array(hi), len(lo), W.wavelet_id, boundary,
                                                J, flags | HOST, c_void_p(ref.ctypes.data)) == 0
            assert np.array_equal(out.reshape(J + 1, B, N), ref)
        for c in range(J + 1):   # and the C restatement, on the last row
            want = O.reconstruct(det[:, B - 1, :], app[B - 1], list(lo), list(hi), boundary, W.wavelet_id,
                                 detail_mask=(1 << (c - 1)) if c else 0, approx_zero=c != 0)
            assert np.array_equal(ref[c, B - 1], want)


def test_malformed_rows_raise(engine, jni):
    B = 12
    x = _signals(B)
    lo, hi = taps(W)
    out = np.zeros((J + 1) * B * N)
    rows = list(x)
    null_late = rows[:10] + [None] + rows[11:]      # in the second chunk: the first chunk has run
    ragged = rows[:9] + [rows[9][:100]] + rows[10:]
    args = lambda r: (r, jni.doubles(lo), jni.doubles(hi), W.wavelet_id, O.PERIODIC, J, 0)  # noqa: E731
    st, _ = jni.call("mraAoS", ctx_of(engine), *args(jni.rows(null_late)), jni.doubles(out),
                     expect=(IAE, "non-null and same length"))
    assert st == 7
    jni.call("mraAoS", ctx_of(engine), *args(jni.rows(ragged)), jni.doubles(out), expect=(IAE, "non-null and same length"))
    jni.call("mraAoS", ctx_of(engine), *args(None), jni.doubles(out), expect=(IAE, "non-null and non-empty"))
    jni.call("mraAoS", ctx_of(engine), *args(jni.rows(x)), jni.doubles(out[:5]), expect=(IAE, "shorter"))
    jni.call("mraAoS", ctx_of(engine), *args(jni.rows(x)), None, expect=(NPE, "output"))
    det = np.zeros((J, B, N))
    tail = (jni.doubles(lo), jni.doubles(hi), W.wavelet_id, O.PERIODIC, 0, jni.doubles(out))
    jni.call("mraPlanesAoS", ctx_of(engine), None, jni.rows(x), *tail, expect=(NPE, "detailPerLevel"))
    jni.call("mraPlanesAoS", ctx_of(engine), jni.planes(det[:, :11]), jni.rows(x), *tail, expect=(IAE, "length=batch"))
    jni.call("mraPlanesAoS", ctx_of(engine), jni.planes(det), jni.rows(ragged), *tail,
             expect=(IAE, "non-null and same length"))
    jni.call("mraPlanesAoS", ctx_of(engine), jni.planes(det), jni.rows(x), jni.doubles(lo), jni.doubles(hi),
             W.wavelet_id, O.PERIODIC, 0, jni.doubles(out[:5]), expect=(IAE, "shorter"))


def test_validation_error_names_the_batch_signal(engine, jni):
    B = 24
    x = _signals(B)
    x[21, 77] = np.nan                               # third chunk (rows 16-23)
    lo, hi = taps(W)
    out = np.zeros((J + 1) * B * N)
    st, pend = jni.call("mraAoS", ctx_of(engine), jni.rows(x), jni.doubles(lo), jni.doubles(hi), W.wavelet_id,
                        O.PERIODIC, J, nat.FLAG_VALIDATE, jni.doubles(out))
    assert st == 3 and pend is None
    msg = jni.last_error()
    assert "non-finite" in msg and "signal 21)" in msg and "index 77" in msg, msg
    assert jni.raw("lastErrorIndex") == 77
