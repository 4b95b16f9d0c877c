"""The inverse-CWT JNI native (icwtAoS in jni/vectorwave_amd_jni.c) through the fake JNIEnv of tests/jni_harness: it
equals the direct C-ABI call on the same planes, table and descriptors, over batches that span several 64 KiB row
chunks (one ending exactly on a chunk, one in a partial chunk), in the SUM form (a band over planes 1..2 of 3) and the
DIRECT form; null and ragged rows, missing tables and short outputs raise; no local reference survives a call
(checked by Jni.call after every native)."""
import numpy as np
import pytest

from test_jni_glue import IAE, NPE, PFX, Jni, _harness, chunk_rows, ctx_of, d, i, l, o
from vectorwave_amd import _native as nat
from vectorwave_amd.cwt import MorletWavelet, build_inverse_tables

pytestmark = pytest.mark.gpu

NATIVES = {"icwtAoS": (i, [l, o, i, o, o, o, i, l, d, i, o])}
SCALES = [0.5, 2.5, 7.0]
S = len(SCALES)


@pytest.fixture(scope="module")
def jni():
    L = _harness()
    for name, (res, args) in NATIVES.items():
        f = getattr(L, PFX + name)
        f.restype, f.argtypes = res, [o, o] + args
    return Jni(L)


def _planes(B, N):
    return np.random.default_rng(B + N).uniform(-1, 1, (B, S, N))


def _args(jni, t):
    desc = np.array([[b, k, w, p] for b, k, w, p, wt, sc in t.scales], dtype=np.int64).ravel()
    wts = np.array([[wt, sc] for b, k, w, p, wt, sc in t.scales], dtype=np.float64).ravel()
    return jni.longs(desc), jni.doubles(wts), jni.doubles(np.array(t.taps)), t.form, t.wrap, t.divisor


@pytest.mark.parametrize("form", ["sum-band", "direct"])
@pytest.mark.parametrize("whole", [True, False], ids=["whole-chunks", "partial-last-chunk"])
def test_native_matches_the_c_abi(engine, jni, form, whole):
    N = 200 if form == "sum-band" else 100
    t = build_inverse_tables(MorletWavelet(), SCALES, N, 1 if form == "sum-band" else 0, S)
    assert t.form == (nat.ICWT_SUM if form == "sum-band" else nat.ICWT_DIRECT)
    cb = chunk_rows((S + 1) * N, 100)
    B = 3 * cb if whole else 2 * cb + 1
    assert cb >= 2 and B > 2 * cb and (B % cb == 0) == whole
    planes = _planes(B, N)
    for flags in (0, nat.FLAG_FMA) if t.form == nat.ICWT_SUM else (0,):
        out = np.full(B * N, -7.0)
        st, pend = jni.call("icwtAoS", ctx_of(engine), jni.rows(planes.reshape(B * S, N)), S, *_args(jni, t), flags,
                            jni.doubles(out))
        assert st == 0 and pend is None, jni.last_error()
        want = engine.icwt(planes, t.scales, t.taps, t.form, t.wrap, t.divisor, flags | nat.FLAG_SYNC)
        assert np.array_equal(out.reshape(B, N), want)
        assert not np.any(out == -7.0)


def test_malformed_arguments_raise(engine, jni):
    N, B = 200, 24
    t = build_inverse_tables(MorletWavelet(), SCALES, N, 0, S)
    planes = _planes(B, N).reshape(B * S, N)
    rows = list(planes)
    out = np.zeros(B * N)
    ok = lambda: _args(jni, t)   # noqa: E731
    cb = chunk_rows((S + 1) * N, B)
    assert cb < 20
    null_late = rows[:60] + [None] + rows[61:]      # past the first chunk: that one has run
    ragged = rows[:59] + [rows[59][:100]] + rows[60:]
    st, _ = jni.call("icwtAoS", ctx_of(engine), jni.rows(null_late), S, *ok(), 0, jni.doubles(out),
                     expect=(IAE, "non-null and same length"))
    assert st == 7
    jni.call("icwtAoS", ctx_of(engine), jni.rows(ragged), S, *ok(), 0, jni.doubles(out), expect=(IAE, "non-null and same length"))
    jni.call("icwtAoS", ctx_of(engine), None, S, *ok(), 0, jni.doubles(out), expect=(IAE, "non-null and non-empty"))
    jni.call("icwtAoS", ctx_of(engine), jni.rows(planes[:B * S - 1]), S, *ok(), 0, jni.doubles(out), expect=(IAE, "S per signal"))
    jni.call("icwtAoS", ctx_of(engine), jni.rows(planes), S, *ok(), 0, jni.doubles(out[:5]), expect=(IAE, "shorter"))
    jni.call("icwtAoS", ctx_of(engine), jni.rows(planes), S, *ok(), 0, None, expect=(NPE, "output"))
    dsc, w, tab, form, wrap, div = ok()
    jni.call("icwtAoS", ctx_of(engine), jni.rows(planes), S, None, w, tab, form, wrap, div, 0, jni.doubles(out), expect=(NPE, "Scales"))
    jni.call("icwtAoS", ctx_of(engine), jni.rows(planes), S, dsc, w, None, form, wrap, div, 0, jni.doubles(out), expect=(NPE, "tables"))
    jni.call("icwtAoS", ctx_of(engine), jni.rows(planes), S, jni.longs(np.zeros(5, dtype=np.int64)), w, tab, form, wrap, div, 0,
             jni.doubles(out), expect=(IAE, "4 values"))
    jni.call("icwtAoS", ctx_of(engine), jni.rows(planes), 0, dsc, w, tab, form, wrap, div, 0, jni.doubles(out), expect=(IAE, "empty"))
    bad = np.array([[0, 17, -8, 0], [0, 0, 0, 1], [0, 17, -8, 2]], dtype=np.int64).ravel()
    st, pend = jni.call("icwtAoS", ctx_of(engine), jni.rows(planes), S, jni.longs(bad), w, tab, form, wrap, div, 0,
                        jni.doubles(out), expect=(IAE, "out of range"))
    assert st == 7
    # an argument error of the C ABI comes back as its status, the message in lastError
    st, pend = jni.call("icwtAoS", ctx_of(engine), jni.rows(planes), S, dsc, w, tab, 9, wrap, div, 0, jni.doubles(out))
    assert st == 7 and "form" in jni.last_error()
    st, pend = jni.call("icwtAoS", ctx_of(engine), jni.rows(planes), S, dsc, w, tab, form, wrap, 0.0, 0, jni.doubles(out))
    assert st == 7 and "divisor" in jni.last_error()
