"""The CWT restatement against itself and the reference's own assertions, on the CPU (tests/cwt_restatement.py):

  - the table form (what vw_cwt_* computes, on vectorwave_amd.cwt.build_tables' tables) equals the literal loops of
    analyzeDirect / analyzeDirectComplex bit for bit, fp64 and fp32, all four paddings -- also where the window
    overshoots the signal by more than N (getBoundaryValue's clamps);
  - a unit delta at p gives c[s][tau] == w_s[p - tau + H] bit for bit inside the window and 0 outside;
  - the zero-signal and linearity assertions of CWTMathematicalValidationTest.java:226-310 and the end-point
    agreement of CWTLinearConvolutionTest.java:72-83 at its 0.001;
  - the shifted direct sum of the FFT form equals the literal FFT branch within 1e-11 * max|c|, the reference's own
    FFT-versus-direct tolerance (util/ToleranceConstants.java:104; measured here <= 9e-16 with |c| ~ 1): this pins
    o_s = +H, q_s = sqrt(s) and M;
  - CWTConfig.shouldUseFFT (:180-192), the half support and its clamp at 16 (CWTTransform.java:774-794), the scale
    spaces and the wavelets' pinned values.
"""
import math

import numpy as np
import pytest

import cwt_restatement as R
from vectorwave_amd import _native as nat
from vectorwave_amd.cwt import (CWTConfig, DOGWavelet, MorletWavelet, PaddingStrategy, PaulWavelet, RickerWavelet,
                                ScaleSpace, build_tables, half_support, next_power_of_two, wavelet_support)
from vectorwave_amd.errors import InvalidArgumentException


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _signal(n, seed=3):
    return np.random.default_rng(seed).standard_normal(n)


@pytest.mark.parametrize("pad", list(PaddingStrategy))
@pytest.mark.parametrize("wavelet", [MorletWavelet(), PaulWavelet(4), RickerWavelet(1.0), DOGWavelet(3)],
                         ids=lambda w: w.name())
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_table_form_is_the_literal_direct_loops(pad, wavelet, dtype):
    cfg = CWTConfig(paddingStrategy=pad, fftEnabled=False)
    scales = [0.5, 2.5, 7.0]     # H = 8 (the clamp), 10 .. 28: wider than the 13-sample row -> the clamps to N-1 / 0
    for n in (1, 13, 40):
        x = _signal(n).astype(dtype)
        lit_re, lit_im = R.analyze_direct_literal(x, scales, wavelet, cfg, dtype)
        (tab_re, tab_im), t = R.analyze_tables(x, scales, wavelet, cfg, dtype)
        assert t.form == "direct" and t.ext == pad.value
        assert np.array_equal(bits(tab_re), bits(lit_re))
        assert (tab_im is None) == (lit_im is None) == (not wavelet.isComplex())
        if tab_im is not None:
            assert np.array_equal(bits(tab_im), bits(lit_im))


@pytest.mark.parametrize("wavelet", [MorletWavelet(), RickerWavelet(1.0)], ids=lambda w: w.name())
def test_unit_delta_reads_the_table_back(wavelet):
    n, p = 50, 21
    cfg = CWTConfig(paddingStrategy=PaddingStrategy.ZERO, fftEnabled=False)
    scales = [1.0, 2.5]
    x = np.zeros(n)
    x[p] = 1.0
    (re, im), t = R.analyze_tables(x, scales, wavelet, cfg)
    for s, (begin, K, o, q) in enumerate(t.scales):
        H = t.half[s]
        assert K == 2 * H + 1 and o == -H and q == 1.0
        for tau in range(n):
            k = p - tau + H
            inside = 0 <= k < K
            assert bits(re[s, tau:tau + 1])[0] == (bits(t.taps_re[begin + k:begin + k + 1])[0] if inside else 0)
            if im is not None:
                # (+0.0 + -0.0 = +0.0: compare values where the tap is a signed zero)
                assert im[s, tau] == (t.taps_im[begin + k] if inside else 0.0)


def test_zero_signal_and_linearity_as_the_reference_asserts():
    """CWTMathematicalValidationTest.java:226-267 (linearity, EPSILON * 10 = 1e-2) and :299-317 (zero signal, 1e-3),
    Morlet with the default configuration; N = 16 < 64, so the direct branch."""
    w, cfg = MorletWavelet(), CWTConfig.defaultConfig()
    (re, im), _ = R.analyze_tables(np.zeros(16), [1.0, 2.0], w, cfg)
    assert np.all(np.abs(re) < 1e-3) and np.all(re == 0.0) and np.all(im == 0.0)
    i = np.arange(16)
    s1, s2 = np.sin(2 * np.pi * i / 4), np.cos(2 * np.pi * i / 8)
    (c1, _), _ = R.analyze_tables(s1, [2.0, 4.0], w, cfg)
    (c2, _), _ = R.analyze_tables(s2, [2.0, 4.0], w, cfg)
    (cc, _), _ = R.analyze_tables(2.0 * s1 + 3.0 * s2, [2.0, 4.0], w, cfg)
    assert np.max(np.abs(2.0 * c1 + 3.0 * c2 - cc)) <= 1e-2
    x = np.array([1, 0, -1, 0, 1, 0, -1, 0], dtype=np.float64)       # :269-297
    (cb, _), _ = R.analyze_tables(x, [1.0, 2.0], w, cfg)
    assert cb.shape == (2, 8) and np.any(np.abs(cb) > 1e-10)


def test_end_points_agree_as_the_linear_convolution_test_asserts():
    """CWTLinearConvolutionTest.java:49-84: Morlet, normalisation off, FFT enabled against disabled, an impulse at
    32 of 64, scale 16: the two results agree at both end points within 0.001."""
    w = MorletWavelet(6.0, 1.0)
    x = np.zeros(64)
    x[32] = 1.0
    (a, _), ta = R.analyze_tables(x, [16.0], w, CWTConfig(fftEnabled=True, normalizeAcrossScales=False))
    (b, _), tb = R.analyze_tables(x, [16.0], w, CWTConfig(fftEnabled=False, normalizeAcrossScales=False))
    assert ta.form == tb.form == "direct"     # a complex wavelet never takes analyzeFFT (:74)
    assert abs(a[0][0] - b[0][0]) <= 0.001 and abs(a[0][63] - b[0][63]) <= 0.001
    # :26-47: no circular artefact -- an impulse near the end leaves the beginning alone
    x = np.zeros(128)
    x[123] = 1.0
    (c, ci), _ = R.analyze_tables(x, [8.0], w, CWTConfig(fftEnabled=True, normalizeAcrossScales=False))
    assert abs(c[0][0]) < abs(c[0][123]) * 0.01


@pytest.mark.parametrize("n", [64, 100, 257, 1000])
@pytest.mark.parametrize("wavelet", [RickerWavelet(1.0), DOGWavelet(2), DOGWavelet(3)], ids=lambda w: w.name())
def test_fft_form_is_the_shifted_direct_sum(n, wavelet):
    """The literal analyzeFFT against the table form (o_s = +H, q_s = sqrt(s), wrap = M) within the reference's
    FFT-versus-direct tolerance 1e-11, relative to max|c|."""
    cfg = CWTConfig.defaultConfig()
    scales = [1.0, 2.5, 7.0, 19.0]
    x = _signal(n, seed=n)
    (tab, im), t = R.analyze_tables(x, scales, wavelet, cfg)
    assert im is None and t.form == "fft" and t.ext == nat.CWT_WRAP_ZERO
    assert t.wrap == next_power_of_two(n + max(wavelet_support(wavelet, s) for s in scales) - 1)
    for s, (begin, K, o, q) in enumerate(t.scales):
        assert o == t.half[s] and K == 2 * t.half[s] + 1 and q == math.sqrt(scales[s])
    lit = R.analyze_fft_literal(x, scales, wavelet, cfg)
    err = np.max(np.abs(lit - tab))
    print(f"n={n} {wavelet.name()}: max|fft - sum| = {err:.3e}, max|c| = {np.max(np.abs(lit)):.3f}")
    assert err <= 1e-11 * np.max(np.abs(lit))
    # ... and the branch is NOT the centred zero-padded sum: it differs from it by O(1)
    (cen, _), _ = R.analyze_tables(x, scales, wavelet, CWTConfig(fftEnabled=False, paddingStrategy=PaddingStrategy.ZERO))
    assert np.max(np.abs(cen - lit)) > 1e-3


def test_fft_form_honours_a_configured_fft_size():
    w, n = RickerWavelet(1.0), 40
    cfg = CWTConfig(fftSize=64)            # shouldUseFFT: n >= 32; fftSize = max(64, nextPow2(40 + 16 - 1)) = 64
    x = _signal(n)
    (tab, _), t = R.analyze_tables(x, [1.0, 2.0], w, cfg)
    assert t.form == "fft" and t.wrap == 64
    lit = R.analyze_fft_literal(x, [1.0, 2.0], w, cfg)
    assert np.max(np.abs(lit - tab)) <= 1e-11 * np.max(np.abs(lit))
    big = CWTConfig(fftSize=4096)
    assert not big.shouldUseFFT(2047) and big.shouldUseFFT(2048)
    assert build_tables(w, big, [1.0], 2048).wrap == 4096


def test_should_use_fft():
    """CWTConfig.java:180-192."""
    d = CWTConfig.defaultConfig()
    assert d.fftEnabled and d.normalizeAcrossScales and d.paddingStrategy is PaddingStrategy.REFLECT and d.fftSize == 0
    assert not d.shouldUseFFT(63) and d.shouldUseFFT(64) and d.shouldUseFFT(1 << 20)
    assert not CWTConfig(fftEnabled=False).shouldUseFFT(1 << 20)
    assert CWTConfig(fftSize=100).shouldUseFFT(50) and not CWTConfig(fftSize=100).shouldUseFFT(49)
    assert CWTConfig(fftSize=101).shouldUseFFT(50)       # integer division
    # the branch: complex wavelets stay direct whatever N
    assert build_tables(MorletWavelet(), d, [2.0], 4096).form == "direct"
    assert build_tables(RickerWavelet(), d, [2.0], 63).form == "direct"
    assert build_tables(RickerWavelet(), d, [2.0], 64).form == "fft"


def test_half_support_and_its_clamp():
    """max(16, ceil(8 s bandwidth)) / 2 (CWTTransform.java:774-794)."""
    m = MorletWavelet()                       # bandwidth 1
    assert [half_support(m, s) for s in (0.1, 0.5, 2.0, 2.01, 2.5, 7.0, 19.0, 150.0, 1024.0)] == \
        [8, 8, 8, 8, 10, 28, 76, 600, 4096]
    assert wavelet_support(m, 2.01) == 17     # ceil(16.08) = 17, 17 / 2 = 8
    r = RickerWavelet(2.0)                    # bandwidth 0.5
    assert half_support(r, 4.0) == 8 and half_support(r, 5.0) == 10
    p = PaulWavelet(4)                        # bandwidth 1/3
    assert half_support(p, 7.0) == math.ceil(8 * 7.0 * (1.0 / math.sqrt(9.0))) // 2 == 9
    assert next_power_of_two(0) == 1 and next_power_of_two(1) == 1 and next_power_of_two(64) == 64
    assert next_power_of_two(65) == 128


def test_scale_spaces():
    assert ScaleSpace.linear(1.0, 4.0, 4).getScales() == [1.0, 2.0, 3.0, 4.0]
    lg = ScaleSpace.logarithmic(1.0, 128.0, 32).getScales()
    assert len(lg) == 32 and lg[0] == 1.0 and abs(lg[-1] - 128.0) < 1e-9
    assert all(b > a for a, b in zip(lg, lg[1:]))
    assert ScaleSpace.dyadic(0, 3).getScales() == [1.0, 2.0, 4.0, 8.0]
    assert ScaleSpace.custom([4.0, 1.0, 2.0]).getScales() == [1.0, 2.0, 4.0]
    for bad in (lambda: ScaleSpace.linear(2.0, 1.0, 3), lambda: ScaleSpace.logarithmic(0.0, 1.0, 3),
                lambda: ScaleSpace.dyadic(3, 1), lambda: ScaleSpace.custom([]), lambda: ScaleSpace.custom([1.0, 1.0])):
        with pytest.raises(InvalidArgumentException):
            bad()


def test_wavelet_values():
    """Closed forms of the reference classes at a few points (its normalisation constants included)."""
    m = MorletWavelet()
    assert m.psi(0.0) == (1.0 / math.pow(math.pi, 0.25)) * (1.0 - math.exp(-18.0)) and m.psiImaginary(0.0) == 0.0
    assert m.isComplex() and m.bandwidth() == 1.0 and m.centerFrequency() == 6.0 / (2 * math.pi)
    r = RickerWavelet(1.0)
    assert r.psi(0.0) == 1.0 / math.sqrt(math.pi) and r.psi(1.0) == 0.0 and not r.isComplex()
    p = PaulWavelet(4)
    base = 16 * 24 / math.sqrt(math.pi * 40320.0)
    assert abs(base - 1.0789368501515768) < 1e-15           # the reference's UNCORRECTED_PAUL4_OUTPUT
    assert p.psi(0.0) == base * 0.6961601901812887 and p.psiImaginary(0.0) == 0.0
    assert abs(p.psi(0.0) - 0.7511128827951223) < 1e-15     # ... and its PYWAVELETS_PAUL4_NORM
    assert PaulWavelet(3).psi(0.0) == 0.0 * 1.0 or abs(PaulWavelet(3).psi(0.0)) < 1e-15   # i^3: real part = base imag
    d2 = DOGWavelet(2)
    assert d2.psi(0.0) == 2.0 / (math.sqrt(3.0) * math.pow(math.pi, 0.25)) and d2.psi(1.0) == 0.0
    d3 = DOGWavelet(3)   # sign (+1) * norm * H3(t) * exp(-t^2/2), H3 = 8 t^3 - 12 t
    assert d3.psi(0.5) == (1.0 / math.sqrt(8 * math.sqrt(math.pi) * 6.0)) * (2.0 * 0.5 * (4 * 0.25 - 2.0) - 4.0 * 1.0) \
        * math.exp(-0.125)
    assert d3.bandwidth() == 1.0 / math.sqrt(3) and d3.centerFrequency() == math.sqrt(3) / (2 * math.pi)
    with pytest.raises(InvalidArgumentException):
        PaulWavelet(0)
    with pytest.raises(InvalidArgumentException):
        DOGWavelet(11)
    with pytest.raises(InvalidArgumentException):
        RickerWavelet(0.0)
