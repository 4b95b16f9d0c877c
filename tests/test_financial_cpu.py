"""Financial analytics, the parts that need no GPU: known answers of the CPU restatement
(tests/fin_restatement.py), the ES tick fixture, the config builders' exceptions, the ABI declarations."""
import os
import re

import numpy as np
import pytest

import fin_restatement as R
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd.errors import InvalidStateException
from vectorwave_amd.financial import FinancialAnalysisConfig, FinancialConfig, VolatilityClassification

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ticks_bid_8x2049.npz")
W = vw.Daubechies.DB4
LO, HI = W.lowPassDecomposition(), W.highPassDecomposition()
SYMBOLS = ("vw_fin_analyze_f64", "vw_fin_sharpe_f64", "vw_fin_wavelet_sharpe_f64")


def test_restatement_constant_row():
    out = R.analyze(np.full(64, 101.25), LO, HI, 3.0)
    assert np.array_equal(out, np.zeros(5))  # four metrics 0.0, flag False (and std 0.0)


def test_restatement_two_prices():
    r = R.returns_of([100.0, 101.0])
    assert len(r) == 1
    a, d = R.coefficients([100.0, 101.0], LO, HI)
    flag, std, _ = R.anomaly(d, 3.0)
    assert R.asymmetry(d) == 0.0 and std == 0.0 and flag is False
    assert R.regime_trend(a) == 0.0


def test_restatement_returns_guard():
    # |p[i-1]| <= 1e-10 gives a 0.0 return; otherwise the relative change
    assert np.array_equal(R.returns_of([1e-11, 5.0, 10.0, 5.0]), np.array([0.0, 1.0, -0.5]))


def test_restatement_sharpe_branches():
    assert R.sharpe([0.5, 0.5, 0.5], 0.02) == np.inf
    assert R.sharpe([0.02, 0.02], 0.02) == 0.0
    assert R.sharpe([0.0, 0.0, 0.0], 0.02) == -np.inf
    assert R.sharpe([0.01, 0.03], 0.0) == pytest.approx(0.02 / np.sqrt(2e-4))


def test_tick_fixture():
    p = np.load(FIXTURE)["prices"]
    assert p.shape == (8, 2049) and p.dtype == np.float64
    assert np.all(p * 4 == np.round(p * 4))  # quantised to 0.25
    for row in p:
        _, d = R.coefficients(row, LO, HI)
        assert int((d == 0.0).sum()) >= 1000


def _full_builder():
    return (FinancialAnalysisConfig.builder().crashAsymmetryThreshold(0.7).volatilityLowThreshold(0.5)
            .volatilityHighThreshold(2.0).regimeTrendThreshold(0.02).anomalyDetectionThreshold(3.0)
            .windowSize(252).confidenceLevel(0.95))


def test_analysis_config_builder():
    c = _full_builder().build()
    assert (c.getCrashAsymmetryThreshold(), c.getVolatilityLowThreshold(), c.getVolatilityHighThreshold(),
            c.getRegimeTrendThreshold(), c.getAnomalyDetectionThreshold(), c.getWindowSize(),
            c.getConfidenceLevel()) == (0.7, 0.5, 2.0, 0.02, 3.0, 252, 0.95)
    setters = [("crashAsymmetryThreshold", "Crash asymmetry threshold"),
               ("volatilityLowThreshold", "Volatility low threshold"),
               ("volatilityHighThreshold", "Volatility high threshold"),
               ("regimeTrendThreshold", "Regime trend threshold"),
               ("anomalyDetectionThreshold", "Anomaly detection threshold")]
    for name, label in setters:
        for bad in (0.0, -1.0):
            with pytest.raises(ValueError, match=re.escape(label + " must be positive")):
                getattr(FinancialAnalysisConfig.builder(), name)(bad)
    with pytest.raises(ValueError, match="Window size must be at least 2"):
        FinancialAnalysisConfig.builder().windowSize(1)
    for bad in (0.0, 1.0):
        with pytest.raises(ValueError, match="Confidence level must be between 0.0 and 1.0"):
            FinancialAnalysisConfig.builder().confidenceLevel(bad)
    # every field is required (IllegalStateException), in the reference's order
    with pytest.raises(InvalidStateException, match="Crash asymmetry threshold must be specified"):
        FinancialAnalysisConfig.builder().build()
    b = FinancialAnalysisConfig.builder().crashAsymmetryThreshold(0.7).volatilityLowThreshold(0.5)
    with pytest.raises(InvalidStateException, match="Volatility high threshold must be specified"):
        b.build()
    b = _full_builder()
    b._confidenceLevel = None
    with pytest.raises(InvalidStateException, match="Confidence level must be specified"):
        b.build()
    with pytest.raises(ValueError, match=re.escape("low=2.0, high=2.0")):
        _full_builder().volatilityLowThreshold(2.0).build()


def test_financial_config_and_analyzers_reject_bad_arguments():
    assert FinancialConfig(0.045).getRiskFreeRate() == 0.045
    assert FinancialConfig(0.0) == FinancialConfig(0.0)
    with pytest.raises(ValueError, match=re.escape("Risk-free rate cannot be negative: -0.01")):
        FinancialConfig(-0.01)
    with pytest.raises(ValueError, match="Configuration cannot be null"):
        vw.FinancialAnalyzer(None)
    with pytest.raises(ValueError, match="Financial configuration cannot be null"):
        vw.FinancialWaveletAnalyzer(None)
    fa = vw.FinancialAnalyzer(_full_builder().build())
    assert fa.classifyVolatility(0.1) == VolatilityClassification.LOW
    assert fa.classifyVolatility(1.0) == VolatilityClassification.NORMAL
    assert fa.classifyVolatility(2.5) == VolatilityClassification.HIGH
    assert fa.isCrashRisk(0.71) and not fa.isCrashRisk(0.7)
    assert fa.isRegimeShift(0.03) and not fa.isRegimeShift(0.02)
    t = vw.FinancialWaveletAnalyzer(FinancialConfig(0.02)).getTransform()
    assert isinstance(t.getWavelet(), vw.Haar) and t.getBoundaryMode() == vw.BoundaryMode.PERIODIC


def test_abi_declares_the_financial_calls():
    with open(os.path.join(ROOT, "include", "vectorwave_amd.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"VW_API vw_status %s\(" % name, header), name
        assert name in nat.SIGNATURES
    assert re.search(r"VW_FLAG_TREE_SUMS = 1u << 9", header) and nat.FLAG_TREE_SUMS == 1 << 9
