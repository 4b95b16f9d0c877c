"""vw_cwt_* / CWTTransform.analyze on the GPU against the restatement (tests/cwt_restatement.py) on the SAME tables
(vectorwave_amd.cwt.build_tables -- tests/test_cwt_restatement_cpu.py ties that table form to the reference's loops).

Shapes where k_cwt can break: N in {1, 16, 31, 100, 257, 1000, 4099} (one partial wave .. a partial fifth time tile),
B in {1, 3}, a padded row stride, host memory; scales {0.5 (the support clamp, K = 17), 1.0, 2.5, 7.0, 19.0,
150.0 (K = 1201 for Morlet: wider than most rows, and a second launch of its own LDS class)}; Morlet and Paul-4
(complex), Ricker, DOG-2 and DOG-3 (real); all four paddings in the direct form, the FFT form through a real
wavelet at N >= 64.

  EXACT  every output's bit pattern equals the restatement's (fp64; fp32 against the restatement at numpy.float32
         with tables rounded once).  A NaN is compared as a NaN, not by its payload: which NaN an invalid operation
         yields is the processor's choice (x86 sets the sign bit, gfx950 does not) and IEEE 754 leaves it open.
  FMA    |gpu - restatement| <= 2 K_s u sum_k|w_s[k]| max|x| (over q_s where q_s > 1: the sums pass through that
         division; never wider than the undivided bound), u = 2^-53 or 2^-24: both sums lie within
         gamma_K sum|w||x| of the exact value, so the bound is derived, not tuned.
"""
import functools

import numpy as np
import pytest

import cwt_restatement as R
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd.cwt import (CWTConfig, CWTTransform, DOGWavelet, MorletWavelet, PaddingStrategy, PaulWavelet,
                                RickerWavelet, build_tables)

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

SCALES = [0.5, 1.0, 2.5, 7.0, 19.0, 150.0]
NS = [1, 16, 31, 100, 257, 1000, 4099]
WAVELETS = {"morlet": MorletWavelet(), "paul4": PaulWavelet(4), "ricker": RickerWavelet(1.0), "dog2": DOGWavelet(2),
            "dog3": DOGWavelet(3)}
REAL = ["ricker", "dog2", "dog3"]
DIRECT = {p: CWTConfig(paddingStrategy=p, fftEnabled=False) for p in PaddingStrategy}
NP = {"f64": np.float64, "f32": np.float32}


@functools.lru_cache(maxsize=None)
def _rows(N, B, dname, ld=None):
    """B rows of N samples (row stride ld), fixed per shape."""
    ld = N if ld is None else ld
    a = np.random.default_rng(1000 * N + B).standard_normal((B, ld)).astype(NP[dname])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _tables(wname, cfg, N):
    return build_tables(WAVELETS[wname], cfg, SCALES, N)


@functools.lru_cache(maxsize=None)
def _expected(wname, cfg, N, B, dname, ld=None):
    """The restatement of every row, computed once per case and shared: (real [B,S,N], imag or None)."""
    t = _tables(wname, cfg, N)
    x = _rows(N, B, dname, ld)
    out = [R.correlate(x[b], N, t.scales, t.taps_re, t.taps_im, t.ext, t.wrap, NP[dname]) for b in range(B)]
    re = np.stack([o[0] for o in out])
    im = None if t.taps_im is None else np.stack([o[1] for o in out])
    re.setflags(write=False)
    return re, im


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _host(a):
    return None if a is None else (a.cpu().numpy() if torch is not None and isinstance(a, torch.Tensor) else np.asarray(a))


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(got.view(u)[~gn], want.view(u)[~wn])


def _check_exact(got_re, got_im, want_re, want_im, what):
    assert _same_bits(_host(got_re), want_re), f"{what}: real plane differs"
    assert (got_im is None) == (want_im is None), what
    if want_im is not None:
        assert _same_bits(_host(got_im), want_im), f"{what}: imaginary plane differs"


# ---- EXACT ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("wname", list(WAVELETS))
def test_direct_form_bit_equal_f64(engine, wname, N):
    for pad, cfg in DIRECT.items():
        for B in (1, 3):
            res = CWTTransform(WAVELETS[wname], cfg).analyze(_dev(_rows(N, B, "f64")), SCALES)
            want = _expected(wname, cfg, N, B, "f64")
            _check_exact(res.getReal(), res.getImaginary(), want[0], want[1], f"{wname} {pad.name} N={N} B={B}")
            assert res.isComplex() == WAVELETS[wname].isComplex() and tuple(res.getReal().shape) == (B, len(SCALES), N)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("wname", ["morlet", "paul4", "ricker", "dog3"])
def test_direct_form_bit_equal_f32(engine, wname, N):
    for pad, cfg in DIRECT.items():
        res = CWTTransform(WAVELETS[wname], cfg).analyze(_dev(_rows(N, 3, "f32")), SCALES)
        assert res.getReal().dtype == torch.float32
        want = _expected(wname, cfg, N, 3, "f32")
        _check_exact(res.getReal(), res.getImaginary(), want[0], want[1], f"{wname} {pad.name} N={N} f32")


@pytest.mark.parametrize("N", [100, 257, 1000, 4099])
@pytest.mark.parametrize("wname", REAL)
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_fft_form_bit_equal(engine, wname, N, dname):
    """A real wavelet at N >= 64 under the default configuration: the shifted sum over the zero-padded period."""
    cfg = CWTConfig.defaultConfig()
    t = _tables(wname, cfg, N)
    assert t.form == "fft" and t.ext == nat.CWT_WRAP_ZERO and t.wrap >= N
    res = CWTTransform(WAVELETS[wname], cfg).analyze(_dev(_rows(N, 3, dname)), SCALES)
    want = _expected(wname, cfg, N, 3, dname)
    _check_exact(res.getReal(), res.getImaginary(), want[0], None, f"{wname} fft N={N} {dname}")


@pytest.mark.parametrize("pad", list(PaddingStrategy))
def test_nonfinite_samples_multiply_every_tap(engine, pad):
    """A NaN and an Inf in one row of three, direct form: every window that reaches them is what the loops give
    (Inf * 0-valued tap = NaN included), the other rows and outputs are untouched."""
    N, cfg = 257, DIRECT[pad]
    x = np.array(_rows(N, 3, "f64"))
    x[1, 40] = np.nan
    x[1, 200] = np.inf
    x[1, 256] = -np.inf
    t = _tables("morlet", cfg, N)
    res = CWTTransform(WAVELETS["morlet"], cfg).analyze(_dev(x), SCALES)
    for b in range(3):
        wr, wi = R.correlate(x[b], N, t.scales, t.taps_re, t.taps_im, t.ext, t.wrap)
        _check_exact(res.getReal()[b], res.getImaginary()[b], wr, wi, f"{pad.name} row {b}")
    assert np.isnan(_host(res.getReal())[1]).any() and not np.isnan(_host(res.getReal())[[0, 2]]).any()


def test_padded_row_stride_and_host_memory(engine):
    """ldx = N + 3 through the raw call; then the same rows from host memory (numpy in, numpy out)."""
    N, B, cfg = 1000, 3, DIRECT[PaddingStrategy.REFLECT]
    t = _tables("morlet", cfg, N)
    x = _rows(N, B, "f64", N + 3)
    want = _expected("morlet", cfg, N, B, "f64", N + 3)
    re, im = engine.cwt(_dev(x), t.scales, t.taps_re, t.taps_im, t.ext, t.wrap, 0, N=N)
    _check_exact(re, im, want[0], want[1], "ldx = N + 3")
    re, im = engine.cwt(np.array(x), t.scales, t.taps_re, t.taps_im, t.ext, t.wrap, 0, N=N)
    assert isinstance(re, np.ndarray)
    _check_exact(re, im, want[0], want[1], "host memory, ldx = N + 3")
    res = CWTTransform(WAVELETS["ricker"], CWTConfig.defaultConfig()).analyze(np.array(_rows(N, B, "f64")), SCALES)
    assert isinstance(res.getReal(), np.ndarray)
    _check_exact(res.getReal(), None, _expected("ricker", CWTConfig.defaultConfig(), N, B, "f64")[0], None, "host fft form")


def test_one_scale_of_8193_taps(engine):
    """Morlet at scale 1024: H = 4096, K = 8193, on a row of 1000."""
    N, cfg, w = 1000, DIRECT[PaddingStrategy.REFLECT], MorletWavelet()
    t = build_tables(w, cfg, [1024.0], N)
    assert t.scales[0][1] == 8193
    x = _rows(N, 1, "f64")
    res = CWTTransform(w, cfg).analyze(_dev(x), [1024.0])
    wr, wi = R.correlate(x[0], N, t.scales, t.taps_re, t.taps_im, t.ext, t.wrap)
    _check_exact(res.getReal()[0], res.getImaginary()[0], wr, wi, "K = 8193")


def test_a_scale_too_wide_is_refused_by_name(engine):
    w = MorletWavelet()
    with pytest.raises(NotImplementedError, match="scale 1"):
        CWTTransform(w, DIRECT[PaddingStrategy.ZERO]).analyze(_dev(_rows(100, 1, "f64")), [1.0, 2049.0])


# ---- FMA -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", ["f64", "f32"])
@pytest.mark.parametrize("wname,cfg", [("morlet", DIRECT[PaddingStrategy.REFLECT]), ("paul4", DIRECT[PaddingStrategy.PERIODIC]),
                                       ("dog2", DIRECT[PaddingStrategy.SYMMETRIC]), ("ricker", CWTConfig.defaultConfig())],
                         ids=["morlet-reflect", "paul4-periodic", "dog2-symmetric", "ricker-fft"])
def test_fma_within_the_derived_bound(engine, wname, cfg, dname):
    for N in (31, 1000, 4099):
        t = _tables(wname, cfg, N)
        x = _rows(N, 3, dname)
        res = CWTTransform(WAVELETS[wname], cfg, fma=True).analyze(_dev(x), SCALES)
        want = _expected(wname, cfg, N, 3, dname)
        br, bi = R.fma_bound(t.scales, t.taps_re, t.taps_im, float(np.max(np.abs(x))), NP[dname])
        dr = np.max(np.abs(_host(res.getReal()).astype(np.float64) - want[0].astype(np.float64)), axis=(0, 2))
        print(f"{wname} {dname} N={N}: real diff / bound per scale = {dr / br}")
        assert np.all(dr <= br), (N, dr, br)
        if bi is not None:
            di = np.max(np.abs(_host(res.getImaginary()).astype(np.float64) - want[1].astype(np.float64)), axis=(0, 2))
            assert np.all(di <= bi), (N, di, bi)
        if N == 4099 and dname == "f64":
            assert dr.max() > 0.0   # the FMA build does fuse: some output differs from the separate roundings


# ---- facade --------------------------------------------------------------------------------------------------------
def test_batch_equals_rows_equals_the_raw_call(engine):
    N, B, cfg, w = 257, 3, CWTConfig.defaultConfig(), WAVELETS["morlet"]
    x = _dev(_rows(N, B, "f64"))
    tx = CWTTransform(w, cfg)
    res = tx.analyze(x, SCALES)
    t = _tables("morlet", cfg, N)
    re, im = engine.cwt(x, t.scales, t.taps_re, t.taps_im, t.ext, t.wrap, 0)
    assert torch.equal(re, res.getReal()) and torch.equal(im, res.getImaginary())
    for b in range(B):
        one = tx.analyze(x[b], SCALES)
        assert tuple(one.getReal().shape) == (len(SCALES), N)
        assert torch.equal(one.getReal(), res.getReal()[b]) and torch.equal(one.getImaginary(), res.getImaginary()[b])
    # a second wavelet's tables in between, then the first again: the device tables follow the call
    other = CWTTransform(WAVELETS["paul4"], cfg).analyze(x, SCALES)
    assert not torch.equal(other.getReal(), res.getReal())
    again = tx.analyze(x, SCALES)
    assert torch.equal(again.getReal(), res.getReal()) and torch.equal(again.getImaginary(), res.getImaginary())


def test_a_call_with_resident_tables_replays_from_a_graph(engine):
    """Once a call has put its tables on the device, the same call can be recorded; a call with new tables cannot."""
    N, B, cfg = 257, 3, DIRECT[PaddingStrategy.REFLECT]
    t, other = _tables("morlet", cfg, N), _tables("paul4", cfg, N)
    want = _expected("morlet", cfg, N, B, "f64")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = _dev(_rows(N, B, "f64"))
        step = lambda: engine.cwt(x, t.scales, t.taps_re, t.taps_im, t.ext, t.wrap, 0)   # noqa: E731
        step()
        g = engine.capture(step)
        re, im = g.result
        re.fill_(float("nan"))
        im.fill_(float("nan"))
        g.launch(2)
        torch.cuda.synchronize()
        _check_exact(re, im, want[0], want[1], "graph replay")
        g.close()
        with pytest.raises(vw.InvalidStateException, match="tables"):
            engine.capture(lambda: engine.cwt(x, other.scales, other.taps_re, other.taps_im, other.ext, other.wrap, 0))
        torch.cuda.synchronize()
    engine.bind_torch_stream()


def test_result_accessors_are_numpy_on_the_restated_planes(engine):
    N, B, cfg = 257, 3, CWTConfig.defaultConfig()
    res = CWTTransform(WAVELETS["morlet"], cfg).analyze(_dev(_rows(N, B, "f64")), SCALES)
    wr, wi = _expected("morlet", cfg, N, B, "f64")
    assert res.isComplex() and res.getNumScales() == len(SCALES) and res.getNumSamples() == N and res.getScales() == SCALES
    assert _same_bits(_host(res.getCoefficients()), wr)
    mag = np.sqrt(wr * wr + wi * wi)
    got = _host(res.getMagnitude())
    assert np.all(np.abs(got - mag) <= np.spacing(mag))          # a square root within 1 ulp on either side
    assert np.all(np.abs(_host(res.getPowerSpectrum()) - got * got) == 0.0)   # magnitude times magnitude
    assert np.all(np.abs(_host(res.getPhase()) - np.arctan2(wi, wr)) <= 4 * np.spacing(np.pi))   # atan2: a few ulp of pi
    assert np.array_equal(_host(res.getScalogram(5)), got[..., 5])
    assert _same_bits(_host(res.getTimeSlice(2)), np.ascontiguousarray(wr[:, 2, :]))
    with pytest.raises(IndexError):
        res.getScalogram(N)
    with pytest.raises(IndexError):
        res.getTimeSlice(len(SCALES))
    # a real wavelet: |c|, c * c, no phase
    cfg = DIRECT[PaddingStrategy.ZERO]
    real = CWTTransform(WAVELETS["dog2"], cfg).analyze(_dev(_rows(N, B, "f64")), SCALES)
    wr, wi = _expected("dog2", cfg, N, B, "f64")
    assert wi is None and not real.isComplex() and real.getPhase() is None and real.getImaginary() is None
    assert np.array_equal(_host(real.getMagnitude()), np.abs(wr))
    assert np.array_equal(_host(real.getPowerSpectrum()), np.abs(wr) * np.abs(wr))


def test_validation_is_the_reference_s(engine):
    """validateInputs (CWTTransform.java:450-469)."""
    tx = CWTTransform(WAVELETS["morlet"])
    x = _dev(_rows(100, 1, "f64"))
    for bad in ([], [1.0, 0.0], [-1.0], None):
        with pytest.raises(vw.InvalidArgumentException):
            tx.analyze(x, bad)
    with pytest.raises(vw.InvalidArgumentException):
        tx.analyze(None, [1.0])
    with pytest.raises(vw.InvalidArgumentException):
        tx.analyze(x[:, :0], [1.0])
    with pytest.raises(vw.InvalidArgumentException):
        CWTTransform(None)
