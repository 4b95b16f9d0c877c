"""The JNI natives for biorthogonal banks (modwtForwardBiAoS / modwtInverseBiAoS in jni/vectorwave_amd_jni.c: lo and
hi of different lengths) through the fake JNIEnv of tests/jni_harness, with tests/test_jni_glue.py's helpers: each
native equals the direct C-ABI call (vw_modwt_*_bi_f64, host memory) on the same data over a batch that spans several
row chunks and ends in a partial one, with the same signal base in chunked error messages; the glue's own argument
errors; and the equal-length natives still refuse two lengths."""
import numpy as np
import pytest

from oracle import oracle as O
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import WID_OTHER, get_wavelet

import restatement_bi as R
from test_jni_glue import HOST, IAE, NPE, PFX, Jni, _harness, chunk_rows, ctx_of, signals, i, l, o

BI_NATIVES = {"modwtForwardBiAoS": (i, [l, o, o, o, i, i, i, i, o, o]),
              "modwtInverseBiAoS": (i, [l, o, o, o, o, i, i, i, o])}


@pytest.fixture(scope="module")
def jni():
    L = _harness()
    for name, (res, args) in BI_NATIVES.items():
        f = getattr(L, PFX + name)
        f.restype, f.argtypes = res, [o, o] + args
    return Jni(L)


def analysis(w):
    return np.array(w.lowPassDecomposition()), np.array(w.highPassDecomposition())


def synthesis(w):
    return np.array(w.lowPassReconstruction()), np.array(w.highPassReconstruction())


def cabi_forward_bi(engine, x, lo, hi, boundary, J, flags):
    B, n = x.shape
    det, app = np.empty((J, B, n)), np.empty((B, n))
    st = engine.lib.vw_modwt_forward_bi_f64(engine.ctx, x.ctypes.data, B, n, n, nat.taps_array(lo), len(lo),
                                            nat.taps_array(hi), len(hi), WID_OTHER, boundary, J, flags | HOST,
                                            det.ctypes.data, app.ctypes.data)
    assert st == 0, nat.last_error()
    return det, app


def cabi_inverse_bi(engine, det, app, lo, hi, boundary, flags):
    J, B, n = det.shape
    y = np.empty((B, n))
    st = engine.lib.vw_modwt_inverse_bi_f64(engine.ctx, det.ctypes.data, app.ctypes.data, B, n, nat.taps_array(lo),
                                            len(lo), nat.taps_array(hi), len(hi), WID_OTHER, boundary, J, 0xFFFFFFFF, 0,
                                            flags | HOST, y.ctypes.data)
    return st, y


# ---- argument errors the glue raises itself (no engine call: runs without a GPU, ctx = 0) ------------------
def test_malformed_arguments_raise_their_own_exceptions(jni):
    lo, hi = analysis(get_wavelet("bior4.4"))
    J, n = 3, 256
    x = signals(4, n, 1)
    det, app, y = np.zeros((J, 4, n)), np.zeros((4, n)), np.zeros((4, n))
    fwd = lambda xo, lo_, hi_, do, ao: (0, xo, lo_, hi_, 0, 0, J, 0, do, ao)  # noqa: E731
    st, _ = jni.call("modwtForwardBiAoS", *fwd(jni.rows([x[0], x[1][:100], x[2], x[3]]), jni.doubles(lo), jni.doubles(hi),
                                               jni.planes(det), jni.rows(app)),
                     expect=(IAE, "all signals must be non-null and same length"))
    assert st == 7
    jni.call("modwtForwardBiAoS", *fwd(jni.rows(x), jni.doubles(lo), jni.doubles(hi), jni.planes(det[:2]),
                                       jni.rows(app)), expect=(IAE, "one plane per level"))
    jni.call("modwtForwardBiAoS", *fwd(jni.rows(x), None, jni.doubles(hi), jni.planes(det), jni.rows(app)),
             expect=(NPE, "taps"))
    jni.call("modwtForwardBiAoS", *fwd(jni.rows(x), jni.doubles(np.zeros(65)), jni.doubles(hi), jni.planes(det),
                                       jni.rows(app)), expect=(IAE, "1..64"))
    jni.call("modwtForwardBiAoS", *fwd(jni.rows(x), jni.doubles(lo), jni.doubles(np.zeros(0)), jni.planes(det),
                                       jni.rows(app)), expect=(IAE, "1..64"))
    jni.call("modwtInverseBiAoS", 0, jni.planes(det), jni.rows(app), jni.doubles(hi), jni.doubles(lo), 0, 0, 0,
             jni.rows(y[:2]), expect=(IAE, "one row per signal"))
    jni.call("modwtInverseBiAoS", 0, jni.planes([det[0], det[1][:3], det[2]]), jni.rows(app), jni.doubles(hi),
             jni.doubles(lo), 0, 0, 0, jni.rows(y), expect=(IAE, "detailPerLevel[L]"))
    # the equal-length natives keep refusing two lengths
    jni.call("modwtForwardAoS", *fwd(jni.rows(x), jni.doubles(lo), jni.doubles(hi), jni.planes(det), jni.rows(app)),
             expect=(IAE, "equal length"))


# ---- each new native against the direct C-ABI call (GPU) ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bior4.4", "bior3.9", "rbio1.5"])
@pytest.mark.parametrize("boundary", [O.PERIODIC, O.SYMMETRIC, O.ZERO_PADDING], ids=["P", "S", "Z"])
@pytest.mark.parametrize("flags", [0, nat.FLAG_FMA, nat.FLAG_CORE_LEVELS | nat.FLAG_VALIDATE | nat.FLAG_FFT_SWITCH],
                         ids=["batch", "fma", "core"])
def test_bi_natives_equal_the_c_abi_over_chunks(engine, jni, name, boundary, flags):
    w, n, J, B = get_wavelet(name), 512, 4, 7
    cb = chunk_rows((J + 2) * n, B)
    assert cb == 2 and B % cb != 0  # four chunks, the last one partial
    x = signals(B, n, 3)
    lo, hi = analysis(w)
    det, app = np.full((J, B, n), -7.0), np.full((B, n), -7.0)
    st, pend = jni.call("modwtForwardBiAoS", ctx_of(engine), jni.rows(x), jni.doubles(lo), jni.doubles(hi), WID_OTHER,
                        boundary, J, flags, jni.planes(det), jni.rows(app))
    assert st == 0 and pend is None, jni.last_error()
    d_ref, a_ref = cabi_forward_bi(engine, x, lo, hi, boundary, J, flags)
    assert np.array_equal(det, d_ref) and np.array_equal(app, a_ref)
    if flags == 0:  # ... and the restatement
        dr, ar = R.decompose(x, list(lo), list(hi), boundary, J)
        assert np.array_equal(det, dr) and np.array_equal(app, ar)
    rl, rh = synthesis(w)
    iflags = flags & ~(nat.FLAG_VALIDATE | nat.FLAG_FFT_SWITCH)
    y = np.full((B, n), -7.0)
    st, pend = jni.call("modwtInverseBiAoS", ctx_of(engine), jni.planes(det), jni.rows(app), jni.doubles(rl),
                        jni.doubles(rh), WID_OTHER, boundary, iflags, jni.rows(y))
    st_ref, y_ref = cabi_inverse_bi(engine, d_ref, a_ref, rl, rh, boundary, iflags)
    assert st == st_ref and pend is None
    if boundary == O.ZERO_PADDING and len(rh) < len(rl):   # the reference indexes past its high-pass array
        assert st == 9 and "high-pass" in jni.last_error()   # VW_ERR_UNSUPPORTED -> UnsupportedOperationException
    else:
        assert st == 0 and np.array_equal(y, y_ref)


@pytest.mark.gpu
def test_nonfinite_error_names_the_batch_signal(engine, jni):
    # chunk 2 (rows 4-5) holds the bad sample: the message names signal 5 of the batch, not signal 1 of the chunk
    w, n, J, B = get_wavelet("bior4.4"), 512, 4, 7
    x = signals(B, n, 5)
    x[5, 123] = np.nan
    lo, hi = analysis(w)
    det, app = np.zeros((J, B, n)), np.zeros((B, n))
    st, pend = jni.call("modwtForwardBiAoS", ctx_of(engine), jni.rows(x), jni.doubles(lo), jni.doubles(hi), WID_OTHER, 0,
                        J, nat.FLAG_CORE_LEVELS | nat.FLAG_VALIDATE, jni.planes(det), jni.rows(app))
    assert st == 3 and pend is None
    msg = jni.last_error()
    assert "signal 5" in msg and "index 123" in msg, msg
    assert jni.raw("lastErrorIndex") == 123
