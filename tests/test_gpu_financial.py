"""Financial analytics on the GPU (vw_fin_analyze_f64 / vw_fin_sharpe_f64 / vw_fin_wavelet_sharpe_f64) against
the sequential CPU restatement (tests/fin_restatement.py).

Exact mode is compared bit for bit (signed zeros and infinities included).  VW_FLAG_TREE_SUMS reorders the
sums only; its bars come from summation error analysis, not from the kernel: any order of n terms of one
sign has relative error <= (n-1)u (u = 2^-53), so two orders differ by < 2nu; a square root halves that
(volatility, std: rtol 2nu is generous); the asymmetry ratio sees three such sums (atol 8nu on a value in
[0, 1]).  regimeTrend is a maximum and stays bit-equal.
"""
import functools
import os
from ctypes import c_void_p

import numpy as np
import pytest

import fin_restatement as R
import vectorwave_amd as vw
from oracle import oracle as O
from vectorwave_amd import _native as nat
from vectorwave_amd.financial import FinancialAnalysisConfig, FinancialConfig, VolatilityClassification
from vectorwave_amd.wavelets import Daubechies, Symlet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = Daubechies.DB4
LO, HI = W.lowPassDecomposition(), W.highPassDecomposition()
K = 3.0
U = 2.0 ** -53
ANALYZE_N = [2, 3, 8, 9, 10, 130, 1001, 4097, 16385]


def _same_bits(a, b) -> bool:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _special_rows():
    rng = np.random.default_rng(130)
    walk = R.random_walk(rng, 2, 130)
    tiny = walk[0].copy()
    tiny[40] = 5e-11       # |p| <= 1e-10: the return out of it is 0.0
    return np.stack([np.full(130, 101.25),                       # constant: every coefficient 0.0
                     100.0 * 1.01 ** np.arange(130),             # strictly rising: a sign count can be 0
                     tiny,
                     -walk[1]])                                  # negative prices


@functools.lru_cache(maxsize=None)
def _prices(name):
    if name == "special":
        return _special_rows()
    if name == "ticks":
        return np.load(os.path.join(ROOT, "tests", "golden", "ticks_bid_8x2049.npz"))["prices"]
    return R.random_walk(np.random.default_rng(name), 3, name)


@functools.lru_cache(maxsize=None)
def _reference(name, k=K):
    return R.analyze_batch(_prices(name), LO, HI, k)


@functools.lru_cache(maxsize=None)
def _ratios(name):
    """max |d - mean| / std per row (0 when std is 0)."""
    return [R.anomaly(R.coefficients(row, LO, HI)[1], K)[2] for row in _prices(name)]


def _to(kind, a):
    if kind == "numpy":
        return a
    import torch
    return torch.tensor(a, dtype=torch.float64, device="cuda")


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


# ---- 1. exact mode ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["numpy", "device"])
@pytest.mark.parametrize("name", ANALYZE_N + ["special"])
def test_analyze_exact_bit_equal(engine, name, kind):
    got = _host(engine.fin_analyze(_to(kind, _prices(name)), LO, HI, K))
    ref = _reference(name)
    assert got.shape == ref.shape
    for j, what in enumerate(("asymmetry", "volatility", "regimeTrend", "anomaly", "std")):
        assert _same_bits(got[j], ref[j]), (what, got[j], ref[j])


@pytest.mark.parametrize("kind", ["numpy", "device"])
def test_analyze_leading_dimension(engine, kind):
    p = _prices("special")
    wide = np.full((p.shape[0], 141), np.nan)
    wide[:, :130] = p
    got = _host(engine.fin_analyze(_to(kind, wide), LO, HI, K, N=130))
    assert _same_bits(got, _reference("special"))


# ---- 2. real ticks ------------------------------------------------------------------------------
def test_ticks_exact_and_flags(engine):
    p = _prices("ticks")
    assert _same_bits(engine.fin_analyze(p, LO, HI, K), _reference("ticks"))
    got = engine.fin_analyze(p, LO, HI, 8.0)
    assert _same_bits(got, _reference("ticks", 8.0))
    # the nearest ratio to 8.0 is 7.72 (3.5 % away): the flags are rows 3 and 6
    assert list(np.nonzero(got[3])[0]) == [3, 6]


# ---- 3. tree sums ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["numpy", "device"])
@pytest.mark.parametrize("name", ANALYZE_N + ["special", "ticks"])
def test_analyze_tree_sums(engine, name, kind):
    p = _prices(name)
    n = p.shape[1] - 1
    got = _host(engine.fin_analyze(_to(kind, p), LO, HI, K, flags=nat.FLAG_TREE_SUMS))
    ref = _reference(name)
    rel = lambda j: (np.abs(got[j] - ref[j]) / np.maximum(np.abs(ref[j]), 1e-300)).max() / (n * U)  # noqa: E731
    print(name, kind, "in units of n*u: asymmetry abs", np.abs(got[0] - ref[0]).max() / (n * U), "volatility rel",
          rel(1), "std rel", rel(4))
    assert _same_bits(got[2], ref[2])
    np.testing.assert_allclose(got[1], ref[1], rtol=2 * n * U, atol=0)
    np.testing.assert_allclose(got[4], ref[4], rtol=2 * n * U, atol=0)
    np.testing.assert_allclose(got[0], ref[0], rtol=0, atol=8 * n * U)
    # the flag is a comparison against k * std: only a ratio within rounding of k could flip it
    for ratio in _ratios(name):
        assert abs(ratio - K) / K > 1e-6
    assert np.array_equal(got[3], ref[3])


# ---- 4. Sharpe ------------------------------------------------------------------------------------
WAVELETS = {"haar": vw.Haar(), "db4": Daubechies.DB4, "sym8": Symlet.SYM8}
BOUNDARIES = {"periodic": O.PERIODIC, "symmetric": O.SYMMETRIC, "zero": O.ZERO_PADDING}
RF = (0.0, 0.02)


@functools.lru_cache(maxsize=None)
def _returns(N):
    rng = np.random.default_rng(1000 + N)
    rows = 0.01 * rng.standard_normal((2, N))
    const = np.stack([np.full(N, 0.5), np.full(N, 0.02), np.zeros(N)])  # mean above / equal to / below rf = 0.02
    return np.concatenate([rows, const])


@pytest.mark.parametrize("N", [2, 3, 17, 1000, 4096, 16384])
def test_sharpe_bit_equal(engine, N):
    r = _returns(N)
    for rf in RF:
        ref = np.array([R.sharpe(row, rf) for row in r])
        assert _same_bits(engine.fin_sharpe(r, rf), ref), (rf, ref)
        assert _same_bits(_host(engine.fin_sharpe(_to("device", r), rf)), ref)
    if N == 2:  # the sums of two equal values are exact: the zero-deviation branches
        assert list(engine.fin_sharpe(r, 0.02)[2:]) == [np.inf, 0.0, -np.inf]


@pytest.mark.parametrize("bname", list(BOUNDARIES))
@pytest.mark.parametrize("wname", list(WAVELETS))
@pytest.mark.parametrize("N", [2, 3, 17, 1000, 4096, 16384])
def test_wavelet_sharpe_bit_equal(engine, N, wname, bname):
    w, boundary = WAVELETS[wname], BOUNDARIES[bname]
    lo, hi = w.lowPassDecomposition(), w.highPassDecomposition()
    r = _returns(N)
    for rf in RF:
        ref = np.array([R.wavelet_sharpe(row, lo, hi, boundary, rf) for row in r])
        assert _same_bits(engine.fin_wavelet_sharpe(r, lo, hi, boundary, rf), ref), (rf, ref)
    got = _host(engine.fin_wavelet_sharpe(_to("device", r), lo, hi, boundary, RF[1]))
    assert _same_bits(got, ref)


def test_sharpe_tree_sums(engine):
    r = _returns(1000)[:2]
    lo, hi = vw.Haar().lowPassDecomposition(), vw.Haar().highPassDecomposition()
    n = r.shape[1]
    # (mean - rf) / std: mean and the squared-deviation sum each within 2nu of the sequential ones relative
    # to sum |v| resp. the sum itself; on zero-mean returns the mean's error is absolute, 2nu * mean|v|
    for got, ref in ((engine.fin_sharpe(r, 0.0, nat.FLAG_TREE_SUMS), [R.sharpe(row, 0.0) for row in r]),
                     (engine.fin_wavelet_sharpe(r, lo, hi, O.PERIODIC, 0.0, nat.FLAG_TREE_SUMS),
                      [R.wavelet_sharpe(row, lo, hi, O.PERIODIC, 0.0) for row in r])):
        np.testing.assert_allclose(got, ref, rtol=2 * n * U, atol=4 * n * U)


# ---- 5. errors ------------------------------------------------------------------------------------
def _analyze_raw(engine, prices, B, N, flags, lo=LO, hi=HI):
    p = np.ascontiguousarray(prices, dtype=np.float64)
    out = np.empty((5, max(B, 1)))
    st = engine.lib.vw_fin_analyze_f64(engine.ctx, c_void_p(p.ctypes.data), B, N, N, nat.taps_array(lo),
                                       nat.taps_array(hi), len(lo), K, flags | nat.FLAG_HOST_MEMORY,
                                       c_void_p(out.ctypes.data))
    return st, nat.last_error(), nat.last_error_index()


def _sharpe_raw(engine, r, B, N, flags, wavelet=False):
    r = np.ascontiguousarray(r, dtype=np.float64)
    out = np.empty(max(B, 1))
    if wavelet:
        st = engine.lib.vw_fin_wavelet_sharpe_f64(engine.ctx, c_void_p(r.ctypes.data), B, N, N, nat.taps_array(LO),
                                                  nat.taps_array(HI), len(LO), 0, 0.0, flags | nat.FLAG_HOST_MEMORY,
                                                  c_void_p(out.ctypes.data))
    else:
        st = engine.lib.vw_fin_sharpe_f64(engine.ctx, c_void_p(r.ctypes.data), B, N, N, 0.0,
                                          flags | nat.FLAG_HOST_MEMORY, c_void_p(out.ctypes.data))
    return st, nat.last_error(), nat.last_error_index()


def test_errors(engine):
    ok = _prices(130)
    st, msg, _ = _analyze_raw(engine, np.ones((3, 1)), 3, 1, 0)
    assert st == 7 and "Prices must contain at least 2 elements" in msg
    assert _analyze_raw(engine, ok, 0, 130, 0)[0] == 2                    # B = 0: VW_ERR_EMPTY
    assert _sharpe_raw(engine, np.ones((3, 4)), 0, 4, 0)[0] == 2
    assert _sharpe_raw(engine, np.ones((3, 4)), 3, 0, 0)[0] == 2          # N = 0: VW_ERR_EMPTY
    assert _sharpe_raw(engine, np.ones((3, 4)), 3, 0, 0, wavelet=True)[0] == 2
    for wavelet in (False, True):
        st, msg, _ = _sharpe_raw(engine, np.ones((3, 1)), 3, 1, 0, wavelet)
        assert st == 7 and msg.startswith("Cannot calculate Sharpe ratio with a single return value. At least 2 "
                                          "returns are required to calculate standard deviation (risk).")
    # VW_FLAG_FMA is refused by all three
    assert _analyze_raw(engine, ok, 3, 130, nat.FLAG_FMA)[0] == 7
    assert _sharpe_raw(engine, ok, 3, 130, nat.FLAG_FMA)[0] == 7
    assert _sharpe_raw(engine, ok, 3, 130, nat.FLAG_FMA, wavelet=True)[0] == 7
    # longer than the LDS plane
    assert _analyze_raw(engine, np.ones((1, 16386)), 1, 16386, 0)[0] == 9
    assert _sharpe_raw(engine, np.ones((1, 16385)), 1, 16385, 0)[0] == 9
    assert _sharpe_raw(engine, np.ones((1, 16385)), 1, 16385, 0, wavelet=True)[0] == 9
    # null arguments
    out = np.empty(15)
    assert engine.lib.vw_fin_analyze_f64(engine.ctx, None, 3, 130, 130, nat.taps_array(LO), nat.taps_array(HI), 8, K,
                                         nat.FLAG_HOST_MEMORY, c_void_p(out.ctypes.data)) == 1
    assert engine.lib.vw_fin_sharpe_f64(engine.ctx, c_void_p(ok.ctypes.data), 3, 130, 130, 0.0,
                                        nat.FLAG_HOST_MEMORY, None) == 1
    assert engine.lib.vw_fin_wavelet_sharpe_f64(engine.ctx, c_void_p(ok.ctypes.data), 3, 130, 130, None,
                                                nat.taps_array(HI), 8, 0, 0.0, nat.FLAG_HOST_MEMORY,
                                                c_void_p(out.ctypes.data)) == 1


def test_validate(engine):
    bad = _prices(130).copy()
    bad[1, 5] = np.nan
    bad[2, 3] = np.inf            # a later offender: the first one in row-major order is reported
    st, msg, idx = _analyze_raw(engine, bad, 3, 130, nat.FLAG_VALIDATE)
    assert st == 7 and "Prices must contain only finite values" in msg and "signal 1)" in msg
    assert idx == 1 * 130 + 5
    engine.lib.vw_set_signal_base(40)
    try:
        st, msg, idx = _analyze_raw(engine, bad, 3, 130, nat.FLAG_VALIDATE)
    finally:
        engine.lib.vw_set_signal_base(0)
    assert st == 7 and "signal 41)" in msg and idx == 41 * 130 + 5
    # a return that overflows between two finite prices: transform.forward's validation
    over = _prices(130).copy()
    over[2, 0], over[2, 1] = 1e-9, 1e300
    st, msg, idx = _analyze_raw(engine, over, 3, 130, nat.FLAG_VALIDATE)
    assert st == 3 and "non-finite" in msg and "signal 2)" in msg and idx == 2 * 130 + 0
    # a non-finite price wins over an overflowed return in an earlier row
    over[0, 0], over[0, 1] = 1e-9, 1e300
    over[2, 100] = np.nan
    st, _, idx = _analyze_raw(engine, over, 3, 130, nat.FLAG_VALIDATE)
    assert st == 7 and idx == 2 * 130 + 100
    # the last price of a row is checked too
    last = _prices(130).copy()
    last[0, 129] = -np.inf
    assert _analyze_raw(engine, last, 3, 130, nat.FLAG_VALIDATE)[2] == 129
    # clean input passes; without VALIDATE the bad rows do not stop the call
    assert _analyze_raw(engine, _prices(130), 3, 130, nat.FLAG_VALIDATE)[0] == 0
    assert _analyze_raw(engine, bad, 3, 130, 0)[0] == 0
    got = engine.fin_analyze(bad, LO, HI, K)
    assert _same_bits(got[:, 0], _reference(130)[:, 0])   # the clean row is unaffected
    # wavelet Sharpe validates its input like the single-level forward
    r = _returns(17).copy()
    r[3, 9] = np.nan
    st, _, idx = _sharpe_raw(engine, r, 5, 17, nat.FLAG_VALIDATE, wavelet=True)
    assert st == 3 and idx == 3 * 17 + 9


# ---- 6. capture -----------------------------------------------------------------------------------
def test_capture_replays(engine):
    import torch
    rng = np.random.default_rng(7)
    p1, p2 = R.random_walk(rng, 4, 1001), R.random_walk(rng, 4, 1001)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.tensor(p1, dtype=torch.float64, device="cuda")
        eager1 = engine.fin_analyze(x, LO, HI, K).clone()
        g = engine.capture(lambda: engine.fin_analyze(x, LO, HI, K))
        g.result.fill_(float("nan"))
        g.launch(1)
        torch.cuda.synchronize()
        assert torch.equal(g.result, eager1)
        x.copy_(torch.tensor(p2, dtype=torch.float64))
        g.launch(1)
        torch.cuda.synchronize()
        eager2 = engine.fin_analyze(x, LO, HI, K)
        torch.cuda.synchronize()
        assert torch.equal(g.result, eager2) and not torch.equal(eager1, eager2)
        g.close()
    assert _same_bits(eager2.cpu().numpy(), R.analyze_batch(p2, LO, HI, K))


# ---- 7. the Python mirror ---------------------------------------------------------------------------
def test_python_mirror(engine):
    cfg = (FinancialAnalysisConfig.builder().crashAsymmetryThreshold(0.7).volatilityLowThreshold(0.5)
           .volatilityHighThreshold(2.0).regimeTrendThreshold(0.02).anomalyDetectionThreshold(8.0)
           .windowSize(252).confidenceLevel(0.95).build())
    fa = vw.FinancialAnalyzer(cfg)
    p = _prices("ticks")
    ref = _reference("ticks", 8.0)
    asym, vol, trend, flags, std = fa.analyzeBatch(p)
    assert _same_bits(asym, ref[0]) and _same_bits(vol, ref[1]) and _same_bits(trend, ref[2])
    assert flags.dtype == bool and list(np.nonzero(flags)[0]) == [3, 6] and _same_bits(std, ref[4])
    assert fa.analyzeCrashAsymmetry(p[3]) == ref[0, 3] and fa.analyzeVolatility(list(p[3])) == ref[1, 3]
    assert fa.analyzeRegimeTrend(p[3]) == ref[2, 3]
    assert fa.detectAnomalies(p[3]) is True and fa.detectAnomalies(p[0]) is False
    assert fa.classifyVolatility(fa.analyzeVolatility(p[0])) == VolatilityClassification.LOW
    tree = fa.analyzeBatch(_to("device", p), tree_sums=True)
    assert _same_bits(tree[2].cpu().numpy(), ref[2]) and list(np.nonzero(tree[3].cpu().numpy())[0]) == [3, 6]
    with pytest.raises(ValueError, match="Prices must contain at least 2 elements"):
        fa.analyzeVolatility([1.0])
    with pytest.raises(ValueError, match="Prices must contain only finite values"):
        fa.analyzeVolatility([1.0, float("nan"), 2.0])
    with pytest.raises(ValueError, match="Prices cannot be null"):
        fa.analyzeVolatility(None)

    r = _returns(1000)
    wa = vw.FinancialWaveletAnalyzer(FinancialConfig(0.02))
    assert wa.calculateSharpeRatio(r[0]) == R.sharpe(r[0], 0.02)
    assert wa.calculateSharpeRatio(r[0], 0.0) == R.sharpe(r[0], 0.0)
    haar = vw.Haar()
    assert wa.calculateWaveletSharpeRatio(r[1]) == R.wavelet_sharpe(r[1], haar.lowPassDecomposition(),
                                                                    haar.highPassDecomposition(), O.PERIODIC, 0.02)
    wb = vw.FinancialWaveletAnalyzer(FinancialConfig(0.0), vw.MODWTTransform(Symlet.SYM8, vw.BoundaryMode.SYMMETRIC))
    s8 = Symlet.SYM8
    ref_w = [R.wavelet_sharpe(row, s8.lowPassDecomposition(), s8.highPassDecomposition(), O.SYMMETRIC, 0.0) for row in r]
    assert _same_bits(wb.calculateWaveletSharpeRatioBatch(r), ref_w)
    assert _same_bits(wb.calculateSharpeRatioBatch(_to("device", r)).cpu().numpy(), [R.sharpe(row, 0.0) for row in r])
    with pytest.raises(ValueError, match="single return value"):
        wa.calculateSharpeRatio([0.01])
    with pytest.raises(ValueError, match="Returns array cannot be null"):
        wa.calculateWaveletSharpeRatio(None)
