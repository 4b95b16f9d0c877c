"""CPU restatement of the financial analytics (test infrastructure, not a test module).

Written from the arithmetic of com.morphiqlabs.financial: FinancialAnalyzer's calculateReturns and its four
reductions over the level-1 PERIODIC MODWT of the returns, FinancialWaveletAnalyzer's Sharpe ratio and its
wavelet-denoised form.  Every sum is a sequential Python float (IEEE binary64) loop in index order, as the
Java loops run; the transforms are the existing oracle's ``modwt_forward`` / ``modwt_inverse``.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as O

EPSILON = 1e-10


def returns_of(prices):
    """r[i-1] = (p[i] - p[i-1]) / p[i-1] when |p[i-1]| > EPSILON, else 0.0."""
    p = [float(v) for v in prices]
    out = []
    for i in range(1, len(p)):
        if abs(p[i - 1]) > EPSILON:
            with np.errstate(all="ignore"):
                out.append(float((np.float64(p[i]) - np.float64(p[i - 1])) / np.float64(p[i - 1])))
        else:
            out.append(0.0)
    return np.array(out, dtype=np.float64)


def coefficients(prices, lo, hi):
    """(approx, detail) of the level-1 PERIODIC MODWT of the returns."""
    return O.modwt_forward(returns_of(prices), lo, hi, O.PERIODIC)


def asymmetry(d) -> float:
    pos = neg = 0.0
    npos = nneg = 0
    for v in (float(t) for t in d):
        if v > 0:
            pos += v
            npos += 1
        elif v < 0:
            neg += abs(v)
            nneg += 1
    if npos == 0 or nneg == 0:
        return 0.0
    pa, na = pos / npos, neg / nneg
    mx = max(pa, na)
    if mx < EPSILON:
        return 0.0
    return abs(na - pa) / mx


def volatility(d) -> float:
    e = 0.0
    for v in (float(t) for t in d):
        e += v * v
    return math.sqrt(e / len(d))


def regime_trend(a) -> float:
    if len(a) < 2:
        return 0.0
    m = 0.0
    for i in range(1, len(a)):
        m = max(m, abs(float(a[i]) - float(a[i - 1])))
    return m


def detail_stats(d):
    """(mean, std) of detectAnomalies: sequential mean, sequential sum of squared deviations, sqrt(var / n)."""
    s = 0.0
    for v in (float(t) for t in d):
        s += v
    mean = s / len(d)
    var = 0.0
    for v in (float(t) for t in d):
        diff = v - mean
        var += diff * diff
    return mean, math.sqrt(var / len(d))


def anomaly(d, k: float):
    """(flag, std, max |d - mean| / std or 0 when std is 0)."""
    mean, std = detail_stats(d)
    flag = any(abs(float(v) - mean) > k * std for v in d)
    dev = max(abs(float(v) - mean) for v in d)
    return flag, std, (dev / std if std > 0 else 0.0)


def analyze(prices, lo, hi, k: float):
    """[asymmetry, volatility, regimeTrend, anomaly (0.0 / 1.0), std] of one price row."""
    a, d = coefficients(prices, lo, hi)
    flag, std, _ = anomaly(d, k)
    return np.array([asymmetry(d), volatility(d), regime_trend(a), 1.0 if flag else 0.0, std])


def analyze_batch(prices, lo, hi, k: float) -> np.ndarray:
    """[5][B] as vw_fin_analyze_f64 lays it out."""
    return np.stack([analyze(row, lo, hi, k) for row in prices], axis=1)


def sharpe(values, rf: float) -> float:
    v = [float(t) for t in values]
    s = 0.0
    for t in v:
        s += t
    mean = s / len(v)
    q = 0.0
    for t in v:
        diff = t - mean
        q += diff * diff
    std = math.sqrt(q / (len(v) - 1))
    if std == 0.0:
        if mean == rf:
            return 0.0
        return math.inf if mean > rf else -math.inf
    return (mean - rf) / std


def wavelet_sharpe(values, lo, hi, boundary: int, rf: float) -> float:
    a, d = O.modwt_forward(values, lo, hi, boundary)
    y = O.modwt_inverse(a, np.zeros_like(d), lo, hi, boundary)
    return sharpe(y, rf)


def random_walk(rng, B: int, N: int) -> np.ndarray:
    """Geometric random-walk prices 100 * exp(cumsum(0.01 * N(0, 1)))."""
    return 100.0 * np.exp(np.cumsum(0.01 * rng.standard_normal((B, N)), axis=1))
