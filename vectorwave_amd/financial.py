"""Financial analytics: Python mirror of ``com.morphiqlabs.financial`` on the HIP engine.

FinancialAnalyzer (crash asymmetry, volatility, regime trend, anomaly detection) and
FinancialWaveletAnalyzer (Sharpe ratio, wavelet-denoised Sharpe ratio) each reduce the level-1 MODWT of a
series to one number.  Here every call is one fused device launch (vw_fin_analyze_f64 / vw_fin_sharpe_f64 /
vw_fin_wavelet_sharpe_f64): the row is read once, the coefficients never leave the compute unit.  The
``...Batch`` forms take ``[B, N]`` (numpy: host-memory path; torch CUDA tensors stay resident) and give every
row exactly what the reference gives that row on its own -- bit for bit unless ``tree_sums`` is set.

Reference: vectorwave-core/src/main/java/com/morphiqlabs/financial/ (FinancialAnalysisConfig.java,
FinancialConfig.java, FinancialAnalyzer.java, FinancialWaveletAnalyzer.java).
"""
from __future__ import annotations

import enum
from typing import Optional

import numpy as np

from . import _native as nat
from .errors import InvalidStateException
from .modwt import BoundaryMode, MODWTTransform, _engine_for
from .wavelets import Daubechies, Haar, require_orthogonal


def _java_double(v: float) -> str:
    """Double.toString for the values the messages print (shortest repr; whole numbers keep '.0')."""
    return repr(float(v))


class FinancialAnalysisConfig:
    """FinancialAnalysisConfig.java: seven required parameters, set through ``builder()``."""

    def __init__(self, builder: "FinancialAnalysisConfig.Builder"):
        required = (("crashAsymmetryThreshold", "Crash asymmetry threshold"),
                    ("volatilityLowThreshold", "Volatility low threshold"),
                    ("volatilityHighThreshold", "Volatility high threshold"),
                    ("regimeTrendThreshold", "Regime trend threshold"),
                    ("anomalyDetectionThreshold", "Anomaly detection threshold"),
                    ("windowSize", "Window size"),
                    ("confidenceLevel", "Confidence level"))
        for attr, label in required:  # :44-64
            if getattr(builder, "_" + attr) is None:
                raise InvalidStateException(f"{label} must be specified")
        if builder._volatilityLowThreshold >= builder._volatilityHighThreshold:  # :67-71
            raise ValueError("Volatility low threshold must be less than high threshold: low=" +
                             _java_double(builder._volatilityLowThreshold) + ", high=" +
                             _java_double(builder._volatilityHighThreshold))
        for attr, _ in required:
            setattr(self, "_" + attr, getattr(builder, "_" + attr))

    @staticmethod
    def builder() -> "FinancialAnalysisConfig.Builder":
        return FinancialAnalysisConfig.Builder()

    def getCrashAsymmetryThreshold(self) -> float:
        return self._crashAsymmetryThreshold

    def getVolatilityLowThreshold(self) -> float:
        return self._volatilityLowThreshold

    def getVolatilityHighThreshold(self) -> float:
        return self._volatilityHighThreshold

    def getRegimeTrendThreshold(self) -> float:
        return self._regimeTrendThreshold

    def getAnomalyDetectionThreshold(self) -> float:
        return self._anomalyDetectionThreshold

    def getWindowSize(self) -> int:
        return self._windowSize

    def getConfidenceLevel(self) -> float:
        return self._confidenceLevel

    class Builder:
        """FinancialAnalysisConfig.Builder :164-288."""

        def __init__(self):
            self._crashAsymmetryThreshold = None
            self._volatilityLowThreshold = None
            self._volatilityHighThreshold = None
            self._regimeTrendThreshold = None
            self._anomalyDetectionThreshold = None
            self._windowSize = None
            self._confidenceLevel = None

        def _positive(self, attr: str, label: str, threshold: float):
            if threshold <= 0:
                raise ValueError(f"{label} must be positive")
            setattr(self, attr, float(threshold))
            return self

        def crashAsymmetryThreshold(self, threshold: float):
            return self._positive("_crashAsymmetryThreshold", "Crash asymmetry threshold", threshold)

        def volatilityLowThreshold(self, threshold: float):
            return self._positive("_volatilityLowThreshold", "Volatility low threshold", threshold)

        def volatilityHighThreshold(self, threshold: float):
            return self._positive("_volatilityHighThreshold", "Volatility high threshold", threshold)

        def regimeTrendThreshold(self, threshold: float):
            return self._positive("_regimeTrendThreshold", "Regime trend threshold", threshold)

        def anomalyDetectionThreshold(self, threshold: float):
            return self._positive("_anomalyDetectionThreshold", "Anomaly detection threshold", threshold)

        def windowSize(self, size: int):
            if size < 2:
                raise ValueError("Window size must be at least 2")
            self._windowSize = int(size)
            return self

        def confidenceLevel(self, level: float):
            if level <= 0.0 or level >= 1.0:
                raise ValueError("Confidence level must be between 0.0 and 1.0")
            self._confidenceLevel = float(level)
            return self

        def build(self) -> "FinancialAnalysisConfig":
            return FinancialAnalysisConfig(self)


class FinancialConfig:
    """FinancialConfig.java: the risk-free rate (an annual decimal), never negative."""

    def __init__(self, riskFreeRate: float):
        if riskFreeRate < 0:
            raise ValueError("Risk-free rate cannot be negative: " + _java_double(riskFreeRate))
        self._riskFreeRate = float(riskFreeRate)

    def getRiskFreeRate(self) -> float:
        return self._riskFreeRate

    def __eq__(self, other):
        return isinstance(other, FinancialConfig) and self._riskFreeRate == other._riskFreeRate

    def __hash__(self):
        return hash(self._riskFreeRate)

    def __repr__(self):
        return "FinancialConfig{riskFreeRate=%.4f}" % self._riskFreeRate


class VolatilityClassification(enum.Enum):
    """FinancialAnalyzer.VolatilityClassification :291-293."""
    LOW = 0
    NORMAL = 1
    HIGH = 2


def _scalar(a, k=None) -> float:
    v = a if k is None else a[k]
    return float(v.reshape(-1)[0].item() if hasattr(v, "reshape") else v)


class FinancialAnalyzer:
    """FinancialAnalyzer.java: DB4, PERIODIC, thresholds from the config.

    The single-series methods return what the reference returns for that series (validatePrices :270-284
    included); ``analyzeBatch`` computes all five numbers for every row of ``[B, N]`` prices in one launch.
    """

    VolatilityClassification = VolatilityClassification

    def __init__(self, config: FinancialAnalysisConfig):
        if config is None:
            raise ValueError("Configuration cannot be null")
        self._config = config
        self._wavelet = Daubechies.DB4
        self._boundary = BoundaryMode.PERIODIC

    def getConfig(self) -> FinancialAnalysisConfig:
        return self._config

    def _run(self, prices, tree_sums: bool = False, validate: bool = True):
        if prices is None:
            raise ValueError("Prices cannot be null")
        if not hasattr(prices, "shape"):
            prices = np.asarray(prices, dtype=np.float64)
        w = self._wavelet
        require_orthogonal(w, "FinancialAnalyzer")
        flags = (nat.FLAG_VALIDATE if validate else 0) | (nat.FLAG_TREE_SUMS if tree_sums else 0)
        return _engine_for(prices).fin_analyze(prices, w.lowPassDecomposition(), w.highPassDecomposition(),
                                               self._config.getAnomalyDetectionThreshold(), flags)

    def analyzeCrashAsymmetry(self, prices) -> float:
        """:52-91."""
        return _scalar(self._run(prices), 0)

    def analyzeVolatility(self, prices) -> float:
        """:103-120."""
        return _scalar(self._run(prices), 1)

    def analyzeRegimeTrend(self, prices) -> float:
        """:132-154."""
        return _scalar(self._run(prices), 2)

    def detectAnomalies(self, prices) -> bool:
        """:166-198."""
        return _scalar(self._run(prices), 3) != 0.0

    def analyzeBatch(self, prices, tree_sums: bool = False, validate: bool = True):
        """All metrics of every row of ``prices[B][N]`` from one launch: ``(asymmetry, volatility,
        regimeTrend, anomaly, detailStd)``, each ``[B]`` (numpy in -> numpy out, device tensor in -> device
        tensors out; ``anomaly`` is boolean).  ``validate=False`` skips the finite checks and the
        synchronisation they need (such a call can be captured into a graph)."""
        out = self._run(prices, tree_sums, validate)
        return out[0], out[1], out[2], out[3] != 0, out[4]

    def classifyVolatility(self, volatility: float) -> VolatilityClassification:
        """:206-214."""
        if volatility < self._config.getVolatilityLowThreshold():
            return VolatilityClassification.LOW
        if volatility > self._config.getVolatilityHighThreshold():
            return VolatilityClassification.HIGH
        return VolatilityClassification.NORMAL

    def isCrashRisk(self, asymmetry: float) -> bool:
        return asymmetry > self._config.getCrashAsymmetryThreshold()

    def isRegimeShift(self, trendChange: float) -> bool:
        return trendChange > self._config.getRegimeTrendThreshold()


class FinancialWaveletAnalyzer:
    """FinancialWaveletAnalyzer.java: Sharpe ratio and wavelet-denoised Sharpe ratio (all details zeroed)."""

    def __init__(self, config: FinancialConfig, transform: Optional[MODWTTransform] = None):
        if config is None:
            raise ValueError("Financial configuration cannot be null")
        if transform is None:
            transform = MODWTTransform(Haar(), BoundaryMode.PERIODIC)  # the one-argument constructor :48-54
        self._config = config
        self._transform = transform

    def getConfig(self) -> FinancialConfig:
        return self._config

    def getTransform(self) -> MODWTTransform:
        return self._transform

    @staticmethod
    def _returns(returns):
        if returns is None:
            raise ValueError("Returns array cannot be null")
        if not hasattr(returns, "shape"):
            returns = np.asarray(returns, dtype=np.float64)
        return returns

    def _rf(self, riskFreeRate):
        return self._config.getRiskFreeRate() if riskFreeRate is None else float(riskFreeRate)

    def calculateSharpeRatioBatch(self, returns, riskFreeRate: Optional[float] = None, tree_sums: bool = False):
        """calculateSharpeRatio :95-124 of every row of ``returns[B][N]`` -> ``[B]``."""
        returns = self._returns(returns)
        return _engine_for(returns).fin_sharpe(returns, self._rf(riskFreeRate),
                                               nat.FLAG_TREE_SUMS if tree_sums else 0)

    def calculateWaveletSharpeRatioBatch(self, returns, riskFreeRate: Optional[float] = None,
                                         tree_sums: bool = False, validate: bool = True):
        """calculateWaveletSharpeRatio :166-212 of every row of ``returns[B][N]`` -> ``[B]``."""
        returns = self._returns(returns)
        t = self._transform
        w = t.getWavelet()
        require_orthogonal(w, "FinancialWaveletAnalyzer.calculateWaveletSharpeRatio")
        flags = (nat.FLAG_VALIDATE if validate else 0) | (nat.FLAG_TREE_SUMS if tree_sums else 0)
        return _engine_for(returns).fin_wavelet_sharpe(returns, w.lowPassDecomposition(), w.highPassDecomposition(),
                                                       int(t.getBoundaryMode()), self._rf(riskFreeRate), flags)

    def calculateSharpeRatio(self, returns, riskFreeRate: Optional[float] = None) -> float:
        return _scalar(self.calculateSharpeRatioBatch(returns, riskFreeRate))

    def calculateWaveletSharpeRatio(self, returns, riskFreeRate: Optional[float] = None) -> float:
        return _scalar(self.calculateWaveletSharpeRatioBatch(returns, riskFreeRate))
