"""The financial JNI natives (finAnalyzeAoS / finSharpeAoS / finWaveletSharpeAoS in jni/vectorwave_amd_jni.c)
through the fake JNIEnv of tests/jni_harness: each native equals the direct C-ABI call on the same rows, over
batches that span several 64 KiB row chunks (one ending exactly on a chunk, one in a partial chunk); null and
ragged rows raise their exceptions; a validation error in a later chunk names the batch's signal; no local
reference survives a call (checked by Jni.call after every native)."""
from ctypes import c_void_p

import numpy as np
import pytest

import fin_restatement as R
from oracle import oracle as O
from test_jni_glue import IAE, NPE, PFX, Jni, _harness, chunk_rows, ctx_of, d, i, l, o, taps
from vectorwave_amd import _native as nat
from vectorwave_amd.financial import FinancialAnalyzer  # noqa: F401  (the feature under test: absent before it)
from vectorwave_amd.wavelets import Daubechies

pytestmark = pytest.mark.gpu

HOST = nat.FLAG_HOST_MEMORY | nat.FLAG_SYNC
NATIVES = {
    "finAnalyzeAoS": (i, [l, o, o, o, d, i, o]),
    "finSharpeAoS": (i, [l, o, d, i, o]),
    "finWaveletSharpeAoS": (i, [l, o, o, o, i, d, i, o]),
}
W = Daubechies.DB4
N = 1001
K = 3.0


@pytest.fixture(scope="module")
def jni():
    L = _harness()
    for name, (res, args) in NATIVES.items():
        f = getattr(L, PFX + name)
        f.restype, f.argtypes = res, [o, o] + args
    return Jni(L)


def _prices(B):
    return R.random_walk(np.random.default_rng(B), B, N)


def _cabi_analyze(engine, p, flags=0):
    B, n = p.shape
    out = np.empty((5, B))
    lo, hi = taps(W)
    st = engine.lib.vw_fin_analyze_f64(engine.ctx, c_void_p(p.ctypes.data), B, n, n, nat.taps_array(lo),
                                       nat.taps_array(hi), len(lo), K, flags | HOST, c_void_p(out.ctypes.data))
    assert st == 0, nat.last_error()
    return out


@pytest.mark.parametrize("B", [40, 43], ids=["whole-chunks", "partial-last-chunk"])
def test_analyze_native_matches_the_c_abi(engine, jni, B):
    cb = chunk_rows(N + 5, B)
    assert cb == 8 and B > 2 * cb and (B % cb != 0) == (B == 43)
    p = _prices(B)
    lo, hi = taps(W)
    for flags in (0, nat.FLAG_TREE_SUMS, nat.FLAG_VALIDATE):
        out = np.full(5 * B, -7.0)
        st, pend = jni.call("finAnalyzeAoS", ctx_of(engine), jni.rows(p), jni.doubles(lo), jni.doubles(hi), K, flags,
                            jni.doubles(out))
        assert st == 0 and pend is None
        assert np.array_equal(out.reshape(5, B), _cabi_analyze(engine, p, flags))
    assert np.array_equal(out.reshape(5, B)[:, B - 1], R.analyze(p[B - 1], lo, hi, K))  # and the restatement


@pytest.mark.parametrize("B", [40, 43], ids=["whole-chunks", "partial-last-chunk"])
def test_sharpe_natives_match_the_c_abi(engine, jni, B):
    assert chunk_rows(N + 1, B) == 8
    r = 0.01 * np.random.default_rng(100 + B).standard_normal((B, N))
    lo, hi = taps(W)
    out, ref = np.full(B, -7.0), np.empty(B)
    st, pend = jni.call("finSharpeAoS", ctx_of(engine), jni.rows(r), 0.02, 0, jni.doubles(out))
    assert st == 0 and pend is None
    assert engine.lib.vw_fin_sharpe_f64(engine.ctx, c_void_p(r.ctypes.data), B, N, N, 0.02, HOST,
                                        c_void_p(ref.ctypes.data)) == 0
    assert np.array_equal(out, ref) and out[B - 1] == R.sharpe(r[B - 1], 0.02)
    for boundary in (O.PERIODIC, O.SYMMETRIC):
        out = np.full(B, -7.0)
        st, pend = jni.call("finWaveletSharpeAoS", ctx_of(engine), jni.rows(r), jni.doubles(lo), jni.doubles(hi),
                            boundary, 0.02, 0, jni.doubles(out))
        assert st == 0 and pend is None
        assert engine.lib.vw_fin_wavelet_sharpe_f64(engine.ctx, c_void_p(r.ctypes.data), B, N, N, nat.taps_array(lo),
                                                    nat.taps_array(hi), len(lo), boundary, 0.02, HOST,
                                                    c_void_p(ref.ctypes.data)) == 0
        assert np.array_equal(out, ref) and out[B - 1] == R.wavelet_sharpe(r[B - 1], lo, hi, boundary, 0.02)


def test_malformed_rows_raise(engine, jni):
    p = _prices(12)
    lo, hi = taps(W)
    out5, out1 = np.zeros(5 * 12), np.zeros(12)
    rows = list(p)
    null_late = rows[:10] + [None] + rows[11:]      # in the second chunk: the first chunk has run
    ragged = rows[:9] + [rows[9][:500]] + rows[10:]
    for name, args, out in (("finAnalyzeAoS", lambda x: (x, jni.doubles(lo), jni.doubles(hi), K, 0), out5),
                            ("finSharpeAoS", lambda x: (x, 0.02, 0), out1),
                            ("finWaveletSharpeAoS", lambda x: (x, jni.doubles(lo), jni.doubles(hi), 0, 0.02, 0), out1)):
        st, _ = jni.call(name, ctx_of(engine), *args(jni.rows(null_late)), jni.doubles(out), expect=(NPE, "cannot be null"))
        assert st == 7
        jni.call(name, ctx_of(engine), *args(jni.rows([None] + rows[1:])), jni.doubles(out), expect=(NPE, "cannot be null"))
        jni.call(name, ctx_of(engine), *args(None), jni.doubles(out), expect=(NPE, "cannot be null"))
        jni.call(name, ctx_of(engine), *args(jni.rows(ragged)), jni.doubles(out), expect=(IAE, "same length"))
        jni.call(name, ctx_of(engine), *args(jni.rows(p)), jni.doubles(out[:5]), expect=(IAE, "shorter"))
        jni.call(name, ctx_of(engine), *args(jni.rows(p)), None, expect=(NPE, "output"))
    jni.call("finAnalyzeAoS", ctx_of(engine), jni.rows(p), jni.doubles(lo), None, K, 0, jni.doubles(out5),
             expect=(NPE, "taps"))
    # the engine's own checks come back as statuses (AmdNative.check throws): one price, one return
    st, pend = jni.call("finAnalyzeAoS", ctx_of(engine), jni.rows(p[:, :1].copy()), jni.doubles(lo), jni.doubles(hi), K,
                        0, jni.doubles(out5))
    assert st == 7 and pend is None and "at least 2 elements" in jni.last_error()
    st, pend = jni.call("finSharpeAoS", ctx_of(engine), jni.rows(p[:, :1].copy()), 0.02, 0, jni.doubles(out1))
    assert st == 7 and pend is None and "single return value" in jni.last_error()


def test_validation_error_names_the_batch_signal(engine, jni):
    B = 40
    p = _prices(B)
    p[21, 77] = np.nan                               # third chunk (rows 16-23)
    lo, hi = taps(W)
    out = np.zeros(5 * B)
    st, pend = jni.call("finAnalyzeAoS", ctx_of(engine), jni.rows(p), jni.doubles(lo), jni.doubles(hi), K,
                        nat.FLAG_VALIDATE, jni.doubles(out))
    assert st == 7 and pend is None
    msg = jni.last_error()
    assert "Prices must contain only finite values" in msg and "signal 21)" in msg and "index 77" in msg, msg
    assert jni.raw("lastErrorIndex") == 21 * N + 77
