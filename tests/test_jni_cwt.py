"""The continuous-wavelet JNI native (cwtAoS in jni/vectorwave_amd_jni.c) through the fake JNIEnv of
tests/jni_harness: it equals the direct C-ABI call on the same rows, tables and descriptors, over batches that span
several 64 KiB row chunks (one ending exactly on a chunk, one in a partial chunk), for a complex table in the direct
form and a real one in the FFT form; null and ragged rows, missing tables and short outputs raise; no local
reference survives a call (checked by Jni.call after every native)."""
import numpy as np
import pytest

from test_jni_glue import IAE, NPE, PFX, Jni, _harness, chunk_rows, ctx_of, i, l, o
from vectorwave_amd import _native as nat
from vectorwave_amd.cwt import CWTConfig, MorletWavelet, RickerWavelet, build_tables

pytestmark = pytest.mark.gpu

NATIVES = {"cwtAoS": (i, [l, o, o, o, o, o, i, l, i, o, o])}
N = 200
SCALES = [0.5, 2.5, 7.0]


@pytest.fixture(scope="module")
def jni():
    L = _harness()
    for name, (res, args) in NATIVES.items():
        f = getattr(L, PFX + name)
        f.restype, f.argtypes = res, [o, o] + args
    return Jni(L)


def _signals(B):
    return np.random.default_rng(B).uniform(-1, 1, (B, N))


def _args(jni, t):
    desc = np.array([[b, k, w] for b, k, w, q in t.scales], dtype=np.int64).ravel()
    div = np.array([q for b, k, w, q in t.scales], dtype=np.float64)
    return (jni.longs(desc), jni.doubles(div), jni.doubles(np.array(t.taps_re)),
            None if t.taps_im is None else jni.doubles(np.array(t.taps_im)), t.ext, t.wrap)


@pytest.mark.parametrize("form", ["direct-complex", "fft-real"])
@pytest.mark.parametrize("whole", [True, False], ids=["whole-chunks", "partial-last-chunk"])
def test_native_matches_the_c_abi(engine, jni, form, whole):
    cplx = form == "direct-complex"
    t = build_tables(MorletWavelet() if cplx else RickerWavelet(), CWTConfig.defaultConfig(), SCALES, N)
    assert t.form == ("direct" if cplx else "fft")
    S = len(SCALES)
    cb = chunk_rows(((2 if cplx else 1) * S + 1) * N, 100)
    B = 3 * cb if whole else 2 * cb + 1
    assert cb >= 2 and B > 2 * cb and (B % cb == 0) == whole
    x = _signals(B)
    for flags in (0, nat.FLAG_FMA):
        out_re = np.full(B * S * N, -7.0)
        out_im = np.full(B * S * N, -7.0) if cplx else None
        st, pend = jni.call("cwtAoS", ctx_of(engine), jni.rows(x), *_args(jni, t), flags, jni.doubles(out_re),
                            None if out_im is None else jni.doubles(out_im))
        assert st == 0 and pend is None, jni.last_error()
        re, im = engine.cwt(x, t.scales, t.taps_re, t.taps_im, t.ext, t.wrap, flags | nat.FLAG_SYNC)
        assert np.array_equal(out_re.reshape(B, S, N), re)
        if cplx:
            assert np.array_equal(out_im.reshape(B, S, N), im)
        assert not np.any(out_re == -7.0)


def test_malformed_arguments_raise(engine, jni):
    t = build_tables(MorletWavelet(), CWTConfig.defaultConfig(), SCALES, N)
    S, B = len(SCALES), 12
    x = _signals(B)
    rows = list(x)
    out = np.zeros(B * S * N)
    ok = lambda: _args(jni, t)   # noqa: E731
    outs = lambda: (jni.doubles(out), jni.doubles(out.copy()))  # noqa: E731
    cb = chunk_rows((2 * S + 1) * N, B)
    assert cb < 10
    null_late = rows[:10] + [None] + rows[11:]      # past the first chunk: that one has run
    ragged = rows[:9] + [rows[9][:100]] + rows[10:]
    st, _ = jni.call("cwtAoS", ctx_of(engine), jni.rows(null_late), *ok(), 0, *outs(), expect=(IAE, "non-null and same length"))
    assert st == 7
    jni.call("cwtAoS", ctx_of(engine), jni.rows(ragged), *ok(), 0, *outs(), expect=(IAE, "non-null and same length"))
    jni.call("cwtAoS", ctx_of(engine), None, *ok(), 0, *outs(), expect=(IAE, "non-null and non-empty"))
    jni.call("cwtAoS", ctx_of(engine), jni.rows(x), *ok(), 0, jni.doubles(out[:5]), jni.doubles(out.copy()),
             expect=(IAE, "shorter"))
    jni.call("cwtAoS", ctx_of(engine), jni.rows(x), *ok(), 0, jni.doubles(out), jni.doubles(out[:5].copy()),
             expect=(IAE, "shorter"))
    jni.call("cwtAoS", ctx_of(engine), jni.rows(x), *ok(), 0, None, jni.doubles(out.copy()), expect=(NPE, "output"))
    d, q, tre, tim, ext, wrap = ok()
    jni.call("cwtAoS", ctx_of(engine), jni.rows(x), None, q, tre, tim, ext, wrap, 0, *outs(), expect=(NPE, "Scales"))
    jni.call("cwtAoS", ctx_of(engine), jni.rows(x), d, q, None, tim, ext, wrap, 0, *outs(), expect=(NPE, "tables"))
    jni.call("cwtAoS", ctx_of(engine), jni.rows(x), jni.longs(np.zeros(5, dtype=np.int64)), q, tre, tim, ext, wrap, 0,
             *outs(), expect=(IAE, "3 values per scale"))
    jni.call("cwtAoS", ctx_of(engine), jni.rows(x), d, q, tre, jni.doubles(np.zeros(3)), ext, wrap, 0, *outs(),
             expect=(IAE, "one length"))
    # an argument error of the C ABI comes back as its status, the message in lastError
    bad = np.array([[0, 17, -8], [0, 0, 0], [0, 17, -8]], dtype=np.int64).ravel()
    st, pend = jni.call("cwtAoS", ctx_of(engine), jni.rows(x), jni.longs(bad), q, tre, tim, ext, wrap, 0, *outs(),
                        expect=(IAE, "out of range"))
    assert st == 7
    st, pend = jni.call("cwtAoS", ctx_of(engine), jni.rows(x), d, q, tre, tim, 9, wrap, 0, *outs())
    assert st == 7 and "extension" in jni.last_error()
