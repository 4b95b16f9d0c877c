"""The inverse CWT's table form against the reference's routes, on the CPU (tests/icwt_restatement.py).

  - the fixed-order sum of VW_ICWT_SUM on build_inverse_tables' tables against the literal FFT route
    (reconstructInternalRealFFT over numpy.fft) for Morlet, Paul-4, Ricker and DOG-2 at N = 128, 200, 256, 1000,
    S = 1, 2, 8, the full range and a band with start > 0: within the reference's own FFT tolerance 1e-11
    (util/ToleranceConstants.java:104) times max(1, max|r|).  The largest difference measured is printed (2.2e-16 at
    max|r| = 0.4 for Morlet; DESIGN.md section 8m records the run);
  - zero-trimmed tables give the untrimmed tables' bits;
  - the direct form on its table equals reconstructInternalRealDirect as written, bit for bit;
  - calculateLogScaleWeights for S = 1, 2, 3; the admissibility constants, the numerical one once (Ricker);
  - every validation message of the facade.
"""
import math

import numpy as np
import pytest

import icwt_restatement as R
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd import cwt as C
from vectorwave_amd.cwt import (CWTResult, DOGWavelet, InverseCWT, MorletWavelet, PaulWavelet, RickerWavelet,
                                build_inverse_tables)

WAVELETS = {"morlet": MorletWavelet(), "paul4": PaulWavelet(4), "ricker": RickerWavelet(1.0), "dog2": DOGWavelet(2)}


def _scales(S):
    return [1.0] if S == 1 else [math.exp(i * math.log(32.0) / (S - 1)) for i in range(S)]


def _planes(S, N, seed=0):
    return np.random.default_rng(100 * N + S + seed).standard_normal((S, N))


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def ricker_numerical():
    return R.admissibility_numerical(WAVELETS["ricker"])


@pytest.mark.parametrize("N", [128, 200, 256, 1000])
@pytest.mark.parametrize("wname", list(WAVELETS))
def test_sum_form_is_what_the_fft_route_computes(wname, N):
    w = WAVELETS[wname]
    c_psi = C.admissibility_constant(w)
    worst = 0.0
    for S in (1, 2, 8):
        scales = _scales(S)
        planes = _planes(S, N)
        for start, end in ((0, S),) + (((1, S),) if S > 1 else ()) + (((2, 6),) if S == 8 else ()):
            t = build_inverse_tables(w, scales, N, start, end)
            assert t.form == nat.ICWT_SUM and t.wrap == C.next_power_of_two(N) and t.divisor == c_psi
            assert [d[3] for d in t.scales] == list(range(start, end))
            got = R.sum_form(planes, N, t.scales, t.taps, t.wrap, t.divisor)
            want = R.reconstruct_fft_literal(planes, scales, N, start, end, w, c_psi)
            diff = float(np.max(np.abs(got - want)))
            bar = R.FFT_TOLERANCE * max(1.0, float(np.max(np.abs(want))))
            worst = max(worst, diff)
            assert diff <= bar, (wname, N, S, start, end, diff, bar)
    print(f"{wname} N={N}: max |sum - fft| = {worst:.3e}")


@pytest.mark.parametrize("wname", list(WAVELETS))
def test_trimmed_tables_give_the_untrimmed_bits(wname):
    w = WAVELETS[wname]
    for N, S in ((128, 2), (200, 8)):
        scales = _scales(S)
        planes = _planes(S, N, 7)
        full = build_inverse_tables(w, scales, N, 0, S, trim=False)
        cut = build_inverse_tables(w, scales, N, 0, S)
        M = full.wrap
        assert all(d[1] == M for d in full.scales)                 # d in (-M/2, M/2]: every entry
        assert all(d[2] == -(M // 2) for d in full.scales)         # o = -d_max = -M/2
        for dtype in (np.float64, np.float32):
            a = R.sum_form(planes, N, full.scales, full.taps, full.wrap, full.divisor, dtype)
            b = R.sum_form(planes, N, cut.scales, cut.taps, cut.wrap, cut.divisor, dtype)
            assert _bits(a, b), (wname, N, dtype)
    if wname == "morlet":   # exp underflows beyond |t| = 38.6: the scale-1 table keeps d in [-38, 38]
        cut = build_inverse_tables(w, [1.0, 64.0], 256, 0, 2)
        assert cut.scales[0][1:3] == (77, -38)
        assert cut.scales[1][1:3] == (256, -128)                   # a large scale is capped by M


@pytest.mark.parametrize("wname", list(WAVELETS))
def test_direct_form_is_the_reference_loop(wname):
    w = WAVELETS[wname]
    c_psi = C.admissibility_constant(w)
    for N, S in ((5, 1), (17, 3), (127, 2)):
        scales = _scales(S) if S > 1 else [0.7]
        planes = _planes(S, N, 3)
        planes[0, 0] = 0.0
        planes[0, N // 2] = 5e-11       # skipped
        planes[-1, N - 1] = -5e-11
        for start, end in ((0, S),) + (((1, S),) if S > 1 else ()):
            t = build_inverse_tables(w, scales, N, start, end)
            assert t.form == nat.ICWT_DIRECT and all(d[1] == 2 * N - 1 for d in t.scales)
            got = R.direct_form(planes, N, t.scales, t.taps, t.divisor)
            want = R.direct_scalar(planes, scales, N, start, end, w, c_psi)
            assert _bits(got, want), (wname, N, S, start)
    # a skipped coefficient is really skipped: with it forced through, the bits change
    N, scales = 17, [1.0, 2.0]
    planes = _planes(2, N, 5) * 1e-9
    planes[1, 3] = 9e-11
    t = build_inverse_tables(w, scales, N, 0, 2)
    with_skip = R.direct_form(planes, N, t.scales, t.taps, t.divisor)
    planes2 = planes.copy()
    planes2[1, 3] = 0.0
    assert _bits(with_skip, R.direct_form(planes2, N, t.scales, t.taps, t.divisor))
    nan = planes.copy()
    nan[0, 2] = np.nan                  # a NaN is not skipped: every output that reads it is NaN
    assert np.isnan(R.direct_form(nan, N, t.scales, t.taps, t.divisor)).all()


def test_log_scale_weights():
    assert C.log_scale_weights([3.5], 0, 1) == [3.5] == R.log_scale_weights([3.5], 0, 1)   # n == 1: the scale itself
    assert C.log_scale_weights([1.0, 3.5, 9.0], 1, 2) == [3.5]
    two = C.log_scale_weights([2.0, 5.0], 0, 2)
    assert two == [math.log(5.0 / 2.0) / 2.0] * 2 == R.log_scale_weights([2.0, 5.0], 0, 2)
    sc = [1.0, 2.5, 7.0, 19.0]
    three = C.log_scale_weights(sc, 1, 4)
    assert three == [math.log(7.0 / 2.5) / 2.0, math.log(19.0 / 2.5) / 2.0, math.log(19.0 / 7.0) / 2.0]
    assert three == R.log_scale_weights(sc, 1, 4)
    assert C.log_scale_weights(sc, 2, 2) == []
    with pytest.raises(vw.InvalidArgumentException, match=r"Scale indices out of bounds: start=0, end=5, scales.length=4"):
        C.log_scale_weights(sc, 0, 5)
    with pytest.raises(vw.InvalidArgumentException,
                       match=r"Scale values must be positive for logarithmic integration. "
                             r"Found non-positive scale at index 1: -2.0"):
        C.log_scale_weights([1.0, -2.0, 3.0], 0, 3)


def test_admissibility_constants(ricker_numerical):
    for w, want in ((MorletWavelet(), math.pi), (DOGWavelet(2), math.pi / math.sqrt(2.0)), (DOGWavelet(3), math.pi),
                    (PaulWavelet(4), 2.0 * math.pi), (PaulWavelet(2), 2.0 * math.pi)):
        inv = InverseCWT(w)
        assert inv.getAdmissibilityConstant() == want == R.admissibility_constant(w) and inv.isAdmissible()
    ricker = RickerWavelet(1.0)
    assert ricker.name() == "ricker1.00"             # no name the reference knows: the numerical fallback
    got = InverseCWT(ricker).getAdmissibilityConstant()
    print(f"ricker C_psi: facade {got!r}, scalar loops {ricker_numerical!r}")
    assert abs(got - ricker_numerical) <= 1e-12 * abs(ricker_numerical)
    assert ricker._admissibility_numerical == got    # cached on the wavelet
    assert InverseCWT(ricker).getAdmissibilityConstant() == got


class _NotAdmissible(C.ContinuousWavelet):
    def name(self):
        return "flat"

    def psi(self, t):
        return 0.0

    def centerFrequency(self):
        return 1.0

    def bandwidth(self):
        return 1.0


def _result(S=3, N=16):
    return CWTResult(np.zeros((S, N)), None, [1.0, 2.0, 4.0][:S], MorletWavelet())


def test_validation_messages():
    inv = InverseCWT(MorletWavelet())
    with pytest.raises(vw.InvalidArgumentException, match="^Wavelet cannot be null$"):
        InverseCWT(None)
    with pytest.raises(vw.InvalidConfigurationException,
                       match=r"^Wavelet does not satisfy admissibility condition: C_ψ = 0.0$"):
        InverseCWT(_NotAdmissible())
    with pytest.raises(vw.InvalidArgumentException, match="^CWT result cannot be null$"):
        inv.reconstruct(None)
    with pytest.raises(vw.InvalidArgumentException, match="^CWT result cannot be null$"):
        inv.reconstructBand(None, 1.0, 2.0)
    with pytest.raises(vw.InvalidArgumentException, match="^CWT result has no scales$"):
        inv.reconstruct(CWTResult(np.zeros((0, 16)), None, [], MorletWavelet()))
    with pytest.raises(vw.InvalidArgumentException, match="^Invalid signal length: 0$"):
        inv.reconstruct(CWTResult(np.zeros((3, 0)), None, [1.0, 2.0, 4.0], MorletWavelet()))
    with pytest.raises(vw.InvalidArgumentException, match="^CWT result has no coefficients$"):
        inv.reconstruct(CWTResult(np.zeros((0, 16)), None, [1.0], MorletWavelet()))
    for lo, hi, text in ((0.0, 2.0, "minScale=0.0, maxScale=2.0"), (-1.0, 2.0, "minScale=-1.0, maxScale=2.0"),
                         (2.0, 2.0, "minScale=2.0, maxScale=2.0"), (3.0, 1.5, "minScale=3.0, maxScale=1.5")):
        with pytest.raises(vw.InvalidArgumentException, match="^Invalid scale range: " + text + "$"):
            inv.reconstructBand(_result(), lo, hi)
    with pytest.raises(vw.InvalidArgumentException, match="^Sampling rate must be positive$"):
        inv.reconstructFrequencyBand(_result(), 0.0, 1.0, 2.0)
    for lo, hi in ((-1.0, 2.0), (2.0, 2.0), (3.0, 1.0), (1.0, 51.0)):
        with pytest.raises(vw.InvalidArgumentException,
                           match=f"^Invalid frequency range: minFreq={lo!r}, maxFreq={hi!r}$"):
            inv.reconstructFrequencyBand(_result(), 100.0, lo, hi)


def test_band_index_search_and_the_empty_band():
    """reconstructBand's index search (:144-161) through the tables it asks for; no scale in range: zeros (:164-167)."""
    asked = []

    class Spy(InverseCWT):
        def _reconstruct(self, coeffs, scales, N, start, end):
            asked.append((start, end))
            return "called"

    inv = Spy(MorletWavelet())
    res = CWTResult(np.ones((5, 16)), None, [1.0, 2.0, 4.0, 8.0, 16.0], MorletWavelet())
    assert inv.reconstruct(res) == "called" and asked[-1] == (0, 5)
    assert inv.reconstructBand(res, 2.0, 8.0) == "called" and asked[-1] == (1, 4)      # max is exclusive past it
    assert inv.reconstructBand(res, 1.5, 7.9) == "called" and asked[-1] == (1, 3)
    assert inv.reconstructBand(res, 0.1, 100.0) == "called" and asked[-1] == (0, 5)
    assert inv.reconstructBand(res, 20.0, 30.0) == "called" and asked[-1] == (0, 5)    # startIdx stays -1: whole range
    n = len(asked)
    zero = inv.reconstructBand(res, 2.5, 3.0)                                          # start 2, end 2: empty
    assert len(asked) == n and isinstance(zero, np.ndarray) and zero.shape == (16,) and not zero.any()
    batch = CWTResult(np.ones((3, 5, 16), dtype=np.float32), None, [1.0, 2.0, 4.0, 8.0, 16.0], MorletWavelet())
    zero = inv.reconstructBand(batch, 2.5, 3.0)
    assert zero.shape == (3, 16) and zero.dtype == np.float32 and not zero.any()
    # frequencies to scales (:200-204): scale = centerFreq * samplingRate / frequency
    cf = MorletWavelet().centerFrequency()
    assert inv.reconstructFrequencyBand(res, 100.0, cf * 100.0 / 12.0, cf * 100.0 / 3.0) == "called"   # scales [3, 12]
    assert asked[-1] == (2, 4)
    assert inv.reconstructFrequencyBand(res, 100.0, 0.0, 50.0) == "called" and asked[-1][1] == 5
