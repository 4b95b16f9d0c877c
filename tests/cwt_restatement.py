"""TEST INFRASTRUCTURE: numpy restatement of the reference's CWTTransform.analyze (cwt/CWTTransform.java).

Two literal restatements, statement by statement:
  analyze_direct_literal   analyzeDirect (:120-169) / analyzeDirectComplex (:174-218) with getBoundaryValue
                           (:354-396): scalar operations of the element type, t ascending, psi evaluated in the loop.
  analyze_fft_literal      analyzeFFT (:223-318): numpy.fft, zero-padding to M, conjugate product, extraction at
                           i + H, division by sqrt(scale).

and the TABLE FORM both reduce to, which is what the C ABI computes (include/vectorwave_amd.h):
  correlate(x, tables)     out[s][tau] = (sum_k w_s[k] * ext(x, tau + o_s + k)) / q_s with k ascending -- one numpy
                           multiply and one numpy add per tap over all tau at once, so every output sees exactly
                           the scalar loop's operations in the scalar loop's order (numpy fuses nothing).
tests/test_cwt_restatement_cpu.py shows the table form equal to the literal loops bit for bit (direct) and within
the reference's own FFT-versus-direct tolerance (FFT); the GPU tests compare against the table form on the same
tables (vectorwave_amd.cwt.build_tables, the helper CWTTransform.analyze itself uses).
"""
import math

import numpy as np

from vectorwave_amd import _native as nat
from vectorwave_amd.cwt import build_tables, half_support, next_power_of_two, wavelet_support


def boundary_index(index, length, ext):
    """getBoundaryValue (:354-396) as the index it reads, None for 0.0; in-range indices read themselves (:147-149)."""
    if 0 <= index < length:
        return index
    if ext == nat.CWT_ZERO:
        return None
    if ext == nat.CWT_REFLECT:
        if index < 0:
            r = -index
            if r >= length:
                r = length - 1
            return r
        r = 2 * length - index - 2
        if r < 0:
            r = 0
        return r
    if ext == nat.CWT_SYMMETRIC:
        if index < 0:
            r = -index - 1
            if r >= length:
                r = length - 1
            return r
        r = 2 * length - index - 1
        if r < 0:
            r = 0
        return r
    if ext == nat.CWT_PERIODIC:
        return (index % length + length) % length   # Java's % keeps the sign; + length, % length again: the same
    raise ValueError(ext)


def analyze_direct_literal(signal, scales, wavelet, config, dtype=np.float64):
    """analyzeDirect / analyzeDirectComplex.  -> (real [S][N], imag [S][N] or None).  dtype float32: the same loops
    on float32 values with the table value rounded once (the fp32 ABI's contract)."""
    x = np.asarray(signal, dtype=dtype)
    n = len(x)
    cplx = wavelet.isComplex()
    re = np.zeros((len(scales), n), dtype=dtype)
    im = np.zeros((len(scales), n), dtype=dtype) if cplx else None
    ext = config.paddingStrategy.value
    for s, scale in enumerate(scales):
        sqrtScale = math.sqrt(scale) if config.normalizeAcrossScales else 1.0
        halfSupport = half_support(wavelet, scale)
        for tau in range(n):
            sumReal = dtype(0.0)
            sumImag = dtype(0.0)
            for t in range(-halfSupport, halfSupport + 1):
                idx = boundary_index(tau + t, n, ext)
                signalValue = dtype(0.0) if idx is None else x[idx]
                waveletReal = dtype(wavelet.psi(-t / scale) / sqrtScale)
                sumReal = dtype(sumReal + dtype(signalValue * waveletReal))
                if cplx:
                    waveletImag = dtype(wavelet.psiImaginary(-t / scale) / sqrtScale)
                    sumImag = dtype(sumImag + dtype(signalValue * waveletImag))
            re[s, tau] = sumReal
            if cplx:
                im[s, tau] = sumImag
    return re, im


def analyze_fft_literal(signal, scales, wavelet, config):
    """analyzeFFT + computeFFTScale + generateScaledWaveletLinear, float64.  -> real [S][N]."""
    x = np.asarray(signal, dtype=np.float64)
    n = len(x)
    maxWaveletSupport = 0
    for scale in scales:
        maxWaveletSupport = max(maxWaveletSupport, wavelet_support(wavelet, scale))
    minFFTSize = n + maxWaveletSupport - 1
    fftSize = max(config.fftSize, next_power_of_two(minFFTSize)) if config.fftSize > 0 else next_power_of_two(minFFTSize)
    padded = np.zeros(fftSize)
    padded[:n] = x
    signalFFT = np.fft.fft(padded)
    out = np.zeros((len(scales), n))
    for s, scale in enumerate(scales):
        sqrtScale = math.sqrt(scale) if config.normalizeAcrossScales else 1.0
        halfSupport = half_support(wavelet, scale)
        waveletArray = np.zeros(fftSize)
        for i in range(2 * halfSupport + 1):
            if i < fftSize:
                waveletArray[i] = wavelet.psi((i - halfSupport) / scale)
        product = signalFFT * np.conj(np.fft.fft(waveletArray))
        convResult = np.fft.ifft(product).real
        for i in range(n):
            idx = i + halfSupport
            out[s, i] = convResult[idx] / sqrtScale if idx < fftSize else 0.0
    return out


def extended_row(x, lo, hi, ext, wrap):
    """ext(x, i) for i in [lo, hi) as an array of x's dtype."""
    n = len(x)
    out = np.zeros(hi - lo, dtype=x.dtype)
    for j, i in enumerate(range(lo, hi)):
        if ext == nat.CWT_WRAP_ZERO:
            m = i % wrap
            if m < n:
                out[j] = x[m]
        else:
            idx = boundary_index(i, n, ext)
            if idx is not None:
                out[j] = x[idx]
    return out


def correlate(x, n, scale_desc, taps_re, taps_im, ext, wrap, dtype=np.float64, fma=False):
    """The table form for ONE row x[:n].  scale_desc: (tap_begin, taps, window_begin, divisor) per scale; the tables
    and the divisor are rounded to dtype once.  -> (real [S][n], imag or None).  fma is not restated (no fused
    operation in numpy): the FMA tests bound the difference instead."""
    assert not fma
    x = np.asarray(x, dtype=dtype)[:n]
    wre = np.asarray(taps_re, dtype=np.float64).astype(dtype)
    wim = None if taps_im is None else np.asarray(taps_im, dtype=np.float64).astype(dtype)
    re = np.zeros((len(scale_desc), n), dtype=dtype)
    im = None if wim is None else np.zeros((len(scale_desc), n), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, (begin, K, o, q) in enumerate(scale_desc):
            xe = extended_row(x, o, n + o + K - 1, ext, wrap)
            acc_r = np.zeros(n, dtype=dtype)
            acc_i = np.zeros(n, dtype=dtype)
            for k in range(K):
                win = xe[k:k + n]
                acc_r = acc_r + win * wre[begin + k]
                if wim is not None:
                    acc_i = acc_i + win * wim[begin + k]
            re[s] = acc_r / dtype(q)
            if wim is not None:
                im[s] = acc_i / dtype(q)
    return re, im


def analyze_tables(signal, scales, wavelet, config, dtype=np.float64):
    """CWTTransform.analyze of one row through build_tables + correlate (what the product computes)."""
    x = np.asarray(signal, dtype=dtype)
    t = build_tables(wavelet, config, list(scales), len(x))
    return correlate(x, len(x), t.scales, t.taps_re, t.taps_im, t.ext, t.wrap, dtype), t


def fma_bound(scale_desc, taps_re, taps_im, max_abs_x, dtype=np.float64):
    """|fma output - separate output| <= 2 K u sum|w| max|x| per scale: both sums lie within gamma_K sum|w||x| of
    the exact sum.  Where the divisor q exceeds 1 (the FFT form at scales above 1) the outputs are the sums over q,
    and so is the bound; it is never wider than the undivided one.
    -> [S] bounds on the real outputs, [S] on the imaginary ones (or None)."""
    u = 2.0 ** -53 if dtype == np.float64 else 2.0 ** -24
    wre = np.abs(np.asarray(taps_re, dtype=np.float64).astype(dtype).astype(np.float64))
    wim = None if taps_im is None else np.abs(np.asarray(taps_im, dtype=np.float64).astype(dtype).astype(np.float64))
    br = np.array([2 * K * u * wre[b:b + K].sum() * max_abs_x / max(float(dtype(q)), 1.0) for b, K, o, q in scale_desc])
    bi = None if wim is None else np.array(
        [2 * K * u * wim[b:b + K].sum() * max_abs_x / max(float(dtype(q)), 1.0) for b, K, o, q in scale_desc])
    return br, bi
