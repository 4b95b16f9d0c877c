"""TEST INFRASTRUCTURE: numpy restatement of the reference's InverseCWT (cwt/InverseCWT.java).

  (a) reconstruct_fft_literal   reconstructInternalRealFFT (:225-270) with createWaveletFFT (:561-586), statement by
                                statement over numpy.fft.
  (b) sum_form                  the fixed-order sum the C ABI's VW_ICWT_SUM computes (include/vectorwave_amd.h),
                                out[tau] = (sum_j weight_j (sum_k w_j[k] z_plane_j[(tau + o_j + k) mod wrap])) / divisor,
                                in the element type: one numpy multiply and one numpy add per tap over all tau at once
                                (EXACT), or one correctly rounded fma per tap and per descriptor through the checker
                                library (FMA; restatement_generic.accumulate).
  (c) direct_literal            reconstructInternalRealDirect (:275-314): the loops over s and b, every t at once --
                                each t sees the scalar loop's operations in the scalar loop's order, and the skip
                                depends on (s, b) alone.
  (d) log_scale_weights, admissibility_numerical, admissibility_constant
                                calculateLogScaleWeights (:411-453), calculateAdmissibilityNumerical (:490-538) and
                                calculateAdmissibilityConstant (:462-485) as scalar loops.
tests/test_icwt_restatement_cpu.py bounds (b) against (a) by the reference's own FFT tolerance; the GPU tests compare
bit for bit against (b) and (c) on the same tables (vectorwave_amd.cwt.build_inverse_tables).
"""
import math

import numpy as np

import restatement_generic as G
from vectorwave_amd import _native as nat
from vectorwave_amd.cwt import ComplexContinuousWavelet, next_power_of_two

DEFAULT_TOLERANCE = 1e-10   # InverseCWT.java:48
FFT_TOLERANCE = 1e-11       # util/ToleranceConstants.java:104


# ---- (d) -----------------------------------------------------------------------------------------------------------
def log_scale_weights(scales, start, end):
    n = end - start
    if n <= 0:
        return []
    weights = [0.0] * n
    if n == 1:
        weights[0] = scales[start]
        return weights
    for i in range(n):
        if i == 0:
            dlogA = math.log(scales[start + 1] / scales[start])
            weights[i] = dlogA / 2.0
        elif i == n - 1:
            dlogA = math.log(scales[start + i] / scales[start + i - 1])
            weights[i] = dlogA / 2.0
        else:
            dlogA = math.log(scales[start + i + 1] / scales[start + i - 1]) / 2.0
            weights[i] = dlogA
    return weights


def wavelet_fourier_transform(wavelet, omega):
    nPoints = 1000
    tMax = 20.0
    dt = 2.0 * tMax / nPoints
    realSum = 0.0
    imagSum = 0.0
    for i in range(nPoints):
        t = -tMax + i * dt
        psi = wavelet.psi(t)
        realSum += psi * math.cos(-omega * t) * dt
        imagSum += psi * math.sin(-omega * t) * dt
    return math.sqrt(realSum * realSum + imagSum * imagSum)


def admissibility_numerical(wavelet):
    nPoints = 10000
    freqs = [0.0] * nPoints
    maxFreq = 100.0
    for i in range(1, nPoints):
        freqs[i] = maxFreq * math.pow(10.0, -4.0 + 4.0 * i / (nPoints - 1))
    total = 0.0
    for i in range(1, nPoints - 1):
        omega = freqs[i]
        psiHat = wavelet_fourier_transform(wavelet, omega)
        integrand = psiHat * psiHat / omega
        dOmega = (freqs[i + 1] - freqs[i - 1]) / 2.0
        total += integrand * dOmega
    return 2.0 * math.pi * total


def admissibility_constant(wavelet):
    name = wavelet.name().lower()
    if "morlet" in name or "morl" in name:
        return math.pi
    if "mexh" in name or "dog2" in name:
        return math.pi / math.sqrt(2.0)
    if "dog" in name:
        return math.pi
    if "paul" in name:
        return 2.0 * math.pi
    if "shannon" in name:
        return math.pi
    return admissibility_numerical(wavelet)


# ---- (a) -----------------------------------------------------------------------------------------------------------
def create_wavelet_time(wavelet, scale, fftSize):
    """createWaveletFFT's waveletTime (:563-576)."""
    waveletTime = np.zeros(fftSize)
    for i in range(fftSize):
        if i <= fftSize // 2:
            t = i / scale
        else:
            t = (i - fftSize) / scale
        waveletTime[i] = wavelet.psi(t) / math.sqrt(scale)
    return waveletTime


def reconstruct_fft_literal(coefficients, scales, signalLength, startScale, endScale, wavelet, admissibility):
    """float64.  coefficients [S][N] -> [N]."""
    fftSize = next_power_of_two(signalLength)
    reconstruction = np.zeros(fftSize, dtype=np.complex128)
    weights = log_scale_weights(scales, startScale, endScale)
    for s in range(startScale, endScale):
        scale = scales[s]
        weight = weights[s - startScale] / scale
        waveletFFT = np.fft.fft(create_wavelet_time(wavelet, scale, fftSize))
        coeff = np.zeros(fftSize)
        coeff[:signalLength] = coefficients[s][:signalLength]
        coeffFFT = np.fft.fft(coeff)
        reconstruction = reconstruction + coeffFFT * waveletFFT * weight
    return np.fft.ifft(reconstruction).real[:signalLength] / admissibility


# ---- (b) -----------------------------------------------------------------------------------------------------------
def sum_form(planes, n, desc, taps, wrap, divisor, dtype=np.float64, fma=False):
    """VW_ICWT_SUM for ONE row's planes [S][>= n].  desc: (tap_begin, taps, window_begin, plane, weight, scale) per
    descriptor; the table, the weights and the divisor are rounded to dtype once.  -> [n]."""
    planes = np.asarray(planes, dtype=dtype)
    w = np.asarray(taps, dtype=np.float64).astype(dtype)
    total = np.zeros(n, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for begin, K, o, plane, weight, _scale in desc:
            idx = np.mod(np.arange(o, o + n + K - 1), wrap)
            live = idx < n
            ze = np.where(live, planes[plane][np.where(live, idx, 0)], dtype(0))
            acc = np.zeros(n, dtype=dtype)
            for k in range(K):
                acc = G.accumulate(acc, ze[k:k + n], w[begin + k], fma)
            total = G.accumulate(total, acc, dtype(weight), fma)
        return total / dtype(divisor)


# ---- (c) -----------------------------------------------------------------------------------------------------------
def reconstruction_kernel(wavelet, t, b, scale):
    """reconstructionKernel (:359-374)."""
    arg = (t - b) / scale
    scaleFactor = 1.0 / math.sqrt(scale)
    if isinstance(wavelet, ComplexContinuousWavelet):
        return scaleFactor * wavelet.psi(arg)
    return scaleFactor * wavelet.psi(arg)


def direct_scalar(coefficients, scales, signalLength, startScale, endScale, wavelet, admissibility):
    """reconstructInternalRealDirect exactly as written, float64, psi evaluated in the loop (small shapes only)."""
    reconstructed = np.zeros(signalLength)
    weights = log_scale_weights(scales, startScale, endScale)
    for t in range(signalLength):
        total = 0.0
        for s in range(startScale, endScale):
            scale = scales[s]
            for b in range(signalLength):
                coeff = float(coefficients[s][b])
                if abs(coeff) < DEFAULT_TOLERANCE:
                    continue
                kernelValue = reconstruction_kernel(wavelet, t, b, scale)
                total += coeff * kernelValue * weights[s - startScale] / scale
        reconstructed[t] = total / admissibility
    return reconstructed


def direct_form(planes, n, desc, taps, divisor, dtype=np.float64):
    """VW_ICWT_DIRECT for ONE row's planes [S][>= n]: the loops of :283-311 over the table w_j[t - b + n - 1], every
    t at once.  -> [n]."""
    planes = np.asarray(planes, dtype=dtype)
    w = np.asarray(taps, dtype=np.float64).astype(dtype)
    tol = dtype(DEFAULT_TOLERANCE)
    t = np.arange(n)
    total = np.zeros(n, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for begin, K, _o, plane, weight, scale in desc:
            assert K == 2 * n - 1
            wt, sc = dtype(weight), dtype(scale)
            for b in range(n):
                coeff = planes[plane][b]
                if abs(coeff) < tol:
                    continue
                total = total + ((coeff * w[begin + t - b + n - 1]) * wt) / sc
        return total / dtype(divisor)


def reconstruct_rows(planes, n, t, dtype=np.float64, fma=False):
    """planes [B][S][>= n] through the tables t (vectorwave_amd.cwt.ICWTTables) -> [B][n]."""
    if t.form == nat.ICWT_SUM:
        rows = [sum_form(p, n, t.scales, t.taps, t.wrap, t.divisor, dtype, fma) for p in planes]
    else:
        rows = [direct_form(p, n, t.scales, t.taps, t.divisor, dtype) for p in planes]
    return np.stack(rows)


def fma_bound(desc, taps, divisor, max_abs_z, dtype=np.float64):
    """|FMA output - EXACT output| for VW_ICWT_SUM, derived as cwt_restatement.fma_bound: per descriptor both inner
    sums lie within K u sum|w| max|z| (to first order, gamma_K) of the exact inner sum, hence within 2 K u sum|w| max|z|
    of each other; the weight carries that through as |weight_j|.  The outer sum adds nsc roundings of a partial sum
    (and, EXACT only, nsc roundings of a product) of magnitude at most A = sum_j |weight_j| sum|w_j| max|z| in either
    mode: 3 nsc u A between the two.  The division is one more rounding of a value at most A / divisor each.
    -> one bound on every output."""
    u = 2.0 ** -53 if dtype == np.float64 else 2.0 ** -24
    w = np.abs(np.asarray(taps, dtype=np.float64).astype(dtype).astype(np.float64))
    inner = sum(abs(float(dtype(wt))) * 2 * K * u * w[b:b + K].sum() * max_abs_z for b, K, o, pl, wt, sc in desc)
    A = sum(abs(float(dtype(wt))) * w[b:b + K].sum() * max_abs_z for b, K, o, pl, wt, sc in desc)
    return (inner + 3 * len(desc) * u * A + 2 * u * A) / float(dtype(divisor))
