"""Continuous wavelet transform: host-side mirror of the reference's ``cwt`` package over vw_cwt_* / vw_icwt_*.

  CWTTransform.analyze, CWTConfig, CWTResult, ScaleSpace          (cwt/)
  InverseCWT.reconstruct / reconstructBand / reconstructFrequencyBand  (cwt/)
  MorletWavelet, RickerWavelet                                    (cwt/)
  PaulWavelet, DOGWavelet                                         (cwt/finance/)

The GPU computes fixed-order correlations of every row with one table per scale (include/vectorwave_amd.h, "continuous
wavelet transform"); this module tabulates the wavelet exactly as the reference's loops evaluate it and picks the
branch as ``CWTTransform.analyze`` (cwt/CWTTransform.java:71-79) does:

  direct   analyzeDirect / analyzeDirectComplex (:120-218): w_s[k] = psi(-(k - H)/s) / sqrtScale, window start -H,
           the padding strategy as the extension.  Complex wavelets always; real ones when not shouldUseFFT(N).
  FFT      analyzeFFT (:223-318), real wavelets when shouldUseFFT(N): the sum that branch's FFTs evaluate,
           c[s][i] = (sum_k psi((k - H)/s) z[(i + H + k) mod M]) / sqrtScale with z = x zero-padded to
           M = nextPow2(N + maxSupport - 1) -- the window starts at i + H, it is NOT centred, and the padding
           strategy is not read.  The GPU evaluates that sum directly; the reference's FFT result differs from it
           by the FFT's own rounding (tests/test_cwt_restatement_cpu.py bounds it at the reference's 1e-11).

``math``'s exp / cos / sin / atan2 / pow may differ from Java's ``Math`` by <= 1 ulp per call, so a table built here
can differ from the Java one in the last bits; the Java facade (AmdCWTTransform) builds its tables with the
wavelet's own ``psi``, so the drop-in is unaffected.  Given a table, the sums are the reference's bit for bit.

The inverse (``InverseCWT``, cwt/InverseCWT.java) always reads the real plane and picks its route as :213 does:

  N >= 128   reconstructInternalRealFFT (:225-270): the weighted sum of circular convolutions over M = nextPowerOfTwo(N)
             that the reference's FFTs evaluate, r[i] = (sum_s wt_s sum_d g_s(d) z_s[(i - d) mod M]) / C_psi with
             g_s(d) = psi(d / a_s) / sqrt(a_s), d in (-M/2, M/2].  The GPU evaluates that sum in a fixed order; a table
             is cut at its outermost non-zero entries, which changes no finite result by a bit.
  N < 128    reconstructInternalRealDirect (:275-314): the reference's loops, term by term.

Not here: analyzeComplex (its direct form divides every term, :523-541, so it is no table correlation),
MODWTBasedInverseCWT, reconstruction from complex coefficients (the reference has none: its ComplexMatrix overload is
dead code), the adaptive scale selectors, the remaining wavelet classes and the cwt/finance analyzers.
"""
from __future__ import annotations

import enum
import math
from decimal import Decimal
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from .engine import Engine
from .errors import InvalidArgumentException, InvalidConfigurationException

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

WAVELET_SUPPORT_FACTOR = 8  # CWTTransform.java:29
FFT_THRESHOLD = 64          # CWTConfig.java:62-91 (default; the reference's property / environment override is not read)


# ---- wavelets --------------------------------------------------------------------------------------------------
class ContinuousWavelet:
    """api/ContinuousWavelet.java: psi, centerFrequency, bandwidth, isComplex."""

    def name(self) -> str:
        raise NotImplementedError

    def psi(self, t: float) -> float:
        raise NotImplementedError

    def centerFrequency(self) -> float:
        raise NotImplementedError

    def bandwidth(self) -> float:
        raise NotImplementedError

    def isComplex(self) -> bool:
        return False


class ComplexContinuousWavelet(ContinuousWavelet):
    """api/ComplexContinuousWavelet.java: psiImaginary; isComplex() is true (:49-51)."""

    def psiImaginary(self, t: float) -> float:
        raise NotImplementedError

    def isComplex(self) -> bool:
        return True


class MorletWavelet(ComplexContinuousWavelet):
    """cwt/MorletWavelet.java."""

    def __init__(self, omega0: float = 6.0, sigma: float = 1.0):
        self.omega0 = float(omega0)
        self.sigma = float(sigma)
        self.normalizationFactor = 1.0 / math.pow(math.pi * self.sigma * self.sigma, 0.25)
        self.correctionTerm = math.exp(-0.5 * self.omega0 * self.omega0 * self.sigma * self.sigma)

    def name(self) -> str:
        return "morl"

    def psi(self, t: float) -> float:
        gaussianEnvelope = math.exp(-0.5 * t * t / (self.sigma * self.sigma))
        carrier = math.cos(self.omega0 * t)
        return self.normalizationFactor * gaussianEnvelope * (carrier - self.correctionTerm)

    def psiImaginary(self, t: float) -> float:
        gaussianEnvelope = math.exp(-0.5 * t * t / (self.sigma * self.sigma))
        carrier = math.sin(self.omega0 * t)
        return self.normalizationFactor * gaussianEnvelope * carrier

    def centerFrequency(self) -> float:
        return self.omega0 / (2 * math.pi)

    def bandwidth(self) -> float:
        return self.sigma


def _factorial(n: int) -> float:
    result = 1.0
    for i in range(2, n + 1):
        result *= i
    return result


class PaulWavelet(ComplexContinuousWavelet):
    """cwt/finance/PaulWavelet.java, its order-4 correction constant included."""

    PAUL4_CORRECTION = 0.6961601901812887

    def __init__(self, m: int = 4):
        if m < 1:
            raise InvalidArgumentException(f"Paul wavelet order must be positive, got: {m}")
        if m > 20:
            raise InvalidArgumentException(f"Paul wavelet order too large (max 20), got: {m}")
        self.m = int(m)
        baseNorm = math.pow(2, m) * _factorial(m) / math.sqrt(math.pi * self._factorial2(2 * m))
        self.normFactor = baseNorm * (self.PAUL4_CORRECTION if m == 4 else 1.0)

    @staticmethod
    def _factorial2(n: int) -> float:  # factorial(): Stirling beyond 20
        if n > 20:
            return math.sqrt(2 * math.pi * n) * math.pow(n / math.e, n)
        return _factorial(n)

    def name(self) -> str:
        return f"paul{self.m}"

    def _complex(self, t: float) -> Tuple[float, float]:
        m = self.m
        modulus = math.sqrt(1 + t * t)
        modulusPow = math.pow(modulus, -(m + 1))
        phase = -(m + 1) * math.atan2(-t, 1.0)
        baseReal = self.normFactor * modulusPow * math.cos(phase)
        baseImag = self.normFactor * modulusPow * math.sin(phase)
        r = m % 4
        if r == 1:
            return -baseImag, baseReal
        if r == 2:
            return -baseReal, -baseImag
        if r == 3:
            return baseImag, -baseReal
        return baseReal, baseImag

    def psi(self, t: float) -> float:
        return self._complex(t)[0]

    def psiImaginary(self, t: float) -> float:
        return self._complex(t)[1]

    def centerFrequency(self) -> float:
        return (2.0 * self.m + 1.0) / (4.0 * math.pi)

    def bandwidth(self) -> float:
        return 1.0 / math.sqrt(2.0 * self.m + 1.0)


class RickerWavelet(ContinuousWavelet):
    """cwt/RickerWavelet.java."""

    SQRT_PI = math.sqrt(math.pi)

    def __init__(self, sigma: float = 1.0):
        if sigma <= 0:
            raise InvalidArgumentException("σ must be positive")
        self.sigma = float(sigma)

    def name(self) -> str:
        return "ricker%.2f" % self.sigma

    def psi(self, t: float) -> float:
        tNorm = t / self.sigma
        tNorm2 = tNorm * tNorm
        return (1 - tNorm2) * math.exp(-tNorm2 / 2) / (self.sigma * self.SQRT_PI)

    def centerFrequency(self) -> float:
        return 1.0 / (2 * math.pi * self.sigma * math.sqrt(2))

    def bandwidth(self) -> float:
        return 1.0 / self.sigma


class DOGWavelet(ContinuousWavelet):
    """cwt/finance/DOGWavelet.java."""

    def __init__(self, n: int = 2):
        if n < 1:
            raise InvalidArgumentException(f"DOG wavelet order must be positive, got: {n}")
        if n > 10:
            raise InvalidArgumentException(f"DOG wavelet order too large (max 10), got: {n}")
        self.n = int(n)
        if n == 2:
            self.normFactor = 2.0 / (math.sqrt(3.0) * math.pow(math.pi, 0.25))
        else:
            self.normFactor = 1.0 / math.sqrt(math.pow(2, n) * math.sqrt(math.pi) * _factorial(n))

    def name(self) -> str:
        return f"dog{self.n}"

    def psi(self, t: float) -> float:
        t_squared = t * t
        if self.n == 2:
            return self.normFactor * (1 - t_squared) * math.exp(-t_squared / 2)
        gaussian = math.exp(-t_squared / 2)
        h0, h1 = 1.0, 2.0 * t           # hermitePolynomial(n, t), n >= 1
        for k in range(2, self.n + 1):
            h0, h1 = h1, 2.0 * t * h1 - 2.0 * (k - 1) * h0
        sign = 1.0 if (self.n + 1) % 2 == 0 else -1.0
        return sign * self.normFactor * h1 * gaussian

    def centerFrequency(self) -> float:
        return math.sqrt(self.n) / (2 * math.pi)

    def bandwidth(self) -> float:
        return 1.0 / math.sqrt(self.n)


# ---- configuration ---------------------------------------------------------------------------------------------
class PaddingStrategy(enum.Enum):
    """CWTConfig.PaddingStrategy, valued as the C ABI's VW_CWT_* extensions."""
    ZERO = nat.CWT_ZERO
    REFLECT = nat.CWT_REFLECT
    SYMMETRIC = nat.CWT_SYMMETRIC
    PERIODIC = nat.CWT_PERIODIC


@dataclass(frozen=True)
class CWTConfig:
    """cwt/CWTConfig.java: the fields CWTTransform.analyze reads (builder defaults, :286-294)."""
    normalizeAcrossScales: bool = True
    paddingStrategy: PaddingStrategy = PaddingStrategy.REFLECT
    fftEnabled: bool = True
    fftSize: int = 0

    def __post_init__(self):
        if self.fftSize < 0:
            raise InvalidArgumentException("FFT size must be non-negative")

    @staticmethod
    def defaultConfig() -> "CWTConfig":
        return CWTConfig()

    def shouldUseFFT(self, signalSize: int) -> bool:
        """CWTConfig.java:180-192."""
        if not self.fftEnabled:
            return False
        if self.fftSize > 0:
            return signalSize >= self.fftSize // 2
        return signalSize >= FFT_THRESHOLD


class ScaleSpace:
    """cwt/ScaleSpace.java."""

    def __init__(self, scales: Sequence[float], kind: str):
        scales = [float(s) for s in scales]
        if not scales:
            raise InvalidArgumentException("Scales array cannot be null or empty")
        for i, s in enumerate(scales):
            if s <= 0:
                raise InvalidArgumentException(f"All scales must be positive, found: {s}")
            if i > 0 and s <= scales[i - 1]:
                raise InvalidArgumentException("Scales must be in ascending order")
        self._scales = scales
        self.type = kind

    @staticmethod
    def _range(minScale: float, maxScale: float, numScales: int) -> None:
        if minScale <= 0 or maxScale <= 0:
            raise InvalidArgumentException("Scales must be positive")
        if minScale >= maxScale:
            raise InvalidArgumentException("minScale must be < maxScale")
        if numScales <= 0:
            raise InvalidArgumentException("Number of scales must be positive")

    @classmethod
    def linear(cls, minScale: float, maxScale: float, numScales: int) -> "ScaleSpace":
        cls._range(minScale, maxScale, numScales)
        step = (maxScale - minScale) / (numScales - 1) if numScales > 1 else math.nan
        return cls([minScale + i * step for i in range(numScales)], "LINEAR")

    @classmethod
    def logarithmic(cls, minScale: float, maxScale: float, numScales: int) -> "ScaleSpace":
        cls._range(minScale, maxScale, numScales)
        logMin, logMax = math.log(minScale), math.log(maxScale)
        logStep = (logMax - logMin) / (numScales - 1) if numScales > 1 else math.nan
        return cls([math.exp(logMin + i * logStep) for i in range(numScales)], "LOGARITHMIC")

    @classmethod
    def dyadic(cls, minLevel: int, maxLevel: int) -> "ScaleSpace":
        if minLevel > maxLevel:
            raise InvalidArgumentException("minLevel must be <= maxLevel")
        return cls([math.pow(2, minLevel + i) for i in range(maxLevel - minLevel + 1)], "DYADIC")

    @classmethod
    def custom(cls, scales: Sequence[float]) -> "ScaleSpace":
        if scales is None or len(scales) == 0:
            raise InvalidArgumentException("Scales array cannot be null or empty")
        return cls(sorted(float(s) for s in scales), "CUSTOM")

    def getScales(self) -> List[float]:
        return list(self._scales)

    def getNumScales(self) -> int:
        return len(self._scales)

    def getMinScale(self) -> float:
        return self._scales[0]

    def getMaxScale(self) -> float:
        return self._scales[-1]

    def getScale(self, index: int) -> float:
        if index < 0 or index >= len(self._scales):
            raise IndexError(f"Scale index out of bounds: {index}")
        return self._scales[index]


# ---- tables ----------------------------------------------------------------------------------------------------
def wavelet_support(wavelet: ContinuousWavelet, scale: float) -> int:
    """CWTTransform.getWaveletSupport (:774-783): max(16, ceil(8 * s * bandwidth))."""
    raw = WAVELET_SUPPORT_FACTOR * scale * wavelet.bandwidth()
    return max(16, min(int(math.ceil(raw)), 2**31 - 1))


def half_support(wavelet: ContinuousWavelet, scale: float) -> int:
    """CWTTransform.getHalfSupport (:792-794)."""
    return wavelet_support(wavelet, scale) // 2


def next_power_of_two(n: int) -> int:
    """CWTTransform.nextPowerOfTwo (:757-766)."""
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


@dataclass
class CWTTables:
    """What one vw_cwt_* call takes, for a wavelet, a configuration, the scales and a row length."""
    form: str                                     # "direct" or "fft"
    scales: List[Tuple[int, int, int, float]]     # (tap_begin, taps, window_begin, divisor) per scale
    taps_re: np.ndarray                           # float64, flat
    taps_im: Optional[np.ndarray]
    ext: int                                      # nat.CWT_*
    wrap: int                                     # the period M of CWT_WRAP_ZERO (0 otherwise)
    half: List[int]                               # H per scale


def validate_scales(scales) -> List[float]:
    """The scale half of CWTTransform.validateInputs (:457-468)."""
    if scales is None:
        raise InvalidArgumentException("Scales cannot be null")
    if isinstance(scales, ScaleSpace):
        scales = scales.getScales()
    scales = [float(s) for s in scales]
    if len(scales) == 0:
        raise InvalidArgumentException("Scales cannot be empty")
    for s in scales:
        if not s > 0:
            raise InvalidArgumentException("All scales must be positive")
    return scales


def build_tables(wavelet: ContinuousWavelet, config: CWTConfig, scales: Sequence[float], N: int) -> CWTTables:
    """The tables and descriptors of CWTTransform.analyze(signal of N samples, scales): the branch as :71-79."""
    cplx = wavelet.isComplex()
    fft = config.shouldUseFFT(N) and not cplx
    norm = config.normalizeAcrossScales
    desc, half, re, im = [], [], [], []
    for s in scales:
        H = half_support(wavelet, s)
        sqrtScale = math.sqrt(s) if norm else 1.0
        begin = len(re)
        if fft:    # generateScaledWaveletLinear (:325-339): psi((i - H)/s); the division follows the sum (:307)
            re.extend(wavelet.psi((i - H) / s) for i in range(2 * H + 1))
            desc.append((begin, 2 * H + 1, H, sqrtScale))
        else:      # :143-155 / :192-211: psi(-t/s) / sqrtScale, t = -H..H
            re.extend(wavelet.psi(-t / s) / sqrtScale for t in range(-H, H + 1))
            if cplx and isinstance(wavelet, ComplexContinuousWavelet):
                im.extend(wavelet.psiImaginary(-t / s) / sqrtScale for t in range(-H, H + 1))
            elif cplx:  # a complex wavelet without psiImaginary: sumImag stays 0.0 (:206-210)
                im.extend(0.0 for _ in range(2 * H + 1))
            desc.append((begin, 2 * H + 1, -H, 1.0))
        half.append(H)
    wrap = 0
    if fft:  # :227-238
        maxSupport = max(wavelet_support(wavelet, s) for s in scales)
        wrap = next_power_of_two(N + maxSupport - 1)
        if config.fftSize > 0:
            wrap = max(config.fftSize, wrap)
    return CWTTables("fft" if fft else "direct", desc, np.asarray(re, dtype=np.float64),
                     np.asarray(im, dtype=np.float64) if cplx else None,
                     nat.CWT_WRAP_ZERO if fft else config.paddingStrategy.value, wrap, half)


# ---- result ----------------------------------------------------------------------------------------------------
class CWTResult:
    """cwt/CWTResult.java over planes [S, N] (one signal) or [B, S, N] (a batch), in the memory the signal was in.
    The derived quantities are elementwise operations on those planes."""

    def __init__(self, real, imag, scales: Sequence[float], wavelet: ContinuousWavelet):
        self.real = real
        self.imag = imag
        self._scales = list(scales)
        self.wavelet = wavelet

    def isComplex(self) -> bool:
        return self.imag is not None

    def getCoefficients(self):
        """The real plane (ComplexMatrix.getReal() for a complex wavelet, CWTResult.java getCoefficients)."""
        return self.real

    def getReal(self):
        return self.real

    def getImaginary(self):
        return self.imag

    def getMagnitude(self):
        """|c| (Math.abs), sqrt(r*r + i*i) for a complex wavelet (ComplexMatrix.getMagnitude :156-166)."""
        if self.imag is None:
            return abs(self.real)
        sq = self.real * self.real + self.imag * self.imag
        return torch.sqrt(sq) if _is_tensor(sq) else np.sqrt(sq)

    def getPhase(self):
        """atan2(imag, real); None for a real wavelet (:getPhase)."""
        if self.imag is None:
            return None
        return torch.atan2(self.imag, self.real) if _is_tensor(self.real) else np.arctan2(self.imag, self.real)

    def getPowerSpectrum(self):
        """magnitude * magnitude (CWTResult.java getPowerSpectrum)."""
        m = self.getMagnitude()
        return m * m

    def getScalogram(self, timeIndex: int):
        if timeIndex < 0 or timeIndex >= self.getNumSamples():
            raise IndexError(f"Time index out of bounds: {timeIndex}")
        return self.getMagnitude()[..., timeIndex]

    def getTimeSlice(self, scaleIndex: int):
        if scaleIndex < 0 or scaleIndex >= self.getNumScales():
            raise IndexError(f"Scale index out of bounds: {scaleIndex}")
        return self.real[..., scaleIndex, :]

    def getScales(self) -> List[float]:
        return list(self._scales)

    def getWavelet(self) -> ContinuousWavelet:
        return self.wavelet

    def getNumScales(self) -> int:
        return len(self._scales)

    def getNumSamples(self) -> int:
        return int(self.real.shape[-1])


def _is_tensor(a) -> bool:
    return torch is not None and isinstance(a, torch.Tensor)


# ---- transform -------------------------------------------------------------------------------------------------
class CWTTransform:
    """cwt/CWTTransform.java analyze(signal, scales) for one signal [N] or a batch [B, N] (numpy: host memory;
    a CUDA tensor: device memory, float64 or float32).  fma=True: one fma per term instead of the reference's
    separate multiply and add."""

    def __init__(self, wavelet: ContinuousWavelet, config: Optional[CWTConfig] = None, fma: bool = False,
                 engine: Optional[Engine] = None):
        if wavelet is None:
            raise InvalidArgumentException("Wavelet cannot be null")
        self.wavelet = wavelet
        self.config = CWTConfig.defaultConfig() if config is None else config
        self.fma = bool(fma)
        self._engine = engine
        self._tables = {}

    def tables(self, scales: Sequence[float], N: int) -> CWTTables:
        key = (tuple(scales), N)
        t = self._tables.get(key)
        if t is None:
            self._tables.clear()   # one shape at a time: a table set can be megabytes
            t = self._tables[key] = build_tables(self.wavelet, self.config, scales, N)
        return t

    def analyze(self, signal, scales) -> CWTResult:
        if signal is None:
            raise InvalidArgumentException("Signal cannot be null")
        shape = tuple(signal.shape) if hasattr(signal, "shape") else np.asarray(signal).shape
        if len(shape) not in (1, 2):
            raise InvalidArgumentException("Signal must be [N] or [B, N]")
        if shape[-1] == 0 or shape[0] == 0:
            raise InvalidArgumentException("Signal cannot be empty")
        scales = validate_scales(scales)
        eng = self._engine
        if eng is None:
            dev = signal.device.index if (_is_tensor(signal) and signal.is_cuda) else None
            eng = Engine.get(dev)
        t = self.tables(scales, int(shape[-1]))
        re, im = eng.cwt(signal, t.scales, t.taps_re, t.taps_im, t.ext, t.wrap, nat.FLAG_FMA if self.fma else 0)
        return CWTResult(re, im, scales, self.wavelet)


# ---- inverse ---------------------------------------------------------------------------------------------------
ICWT_FFT_MIN_LENGTH = 128   # InverseCWT.java:213


def _jd(x: float) -> str:
    """Double.toString for the values the reference's messages print."""
    x = float(x)
    if x != x:
        return "NaN"
    if x in (math.inf, -math.inf):
        return "Infinity" if x > 0 else "-Infinity"
    if x == 0 or 1e-3 <= abs(x) < 1e7:
        return repr(x)
    sign, digits, exp = Decimal(repr(x)).as_tuple()   # the shortest digits that round-trip, as Java prints
    digits = "".join(map(str, digits)).rstrip("0") or "0"
    e = len(Decimal(repr(x)).as_tuple().digits) - 1 + exp
    m = ("-" if sign else "") + digits[0] + "." + (digits[1:] or "0")
    return f"{m}E{e}"


def log_scale_weights(scales: Sequence[float], start: int, end: int) -> List[float]:
    """InverseCWT.calculateLogScaleWeights (:411-453)."""
    n = end - start
    if n <= 0:
        return []
    if start < 0 or end > len(scales):
        raise InvalidArgumentException(
            f"Scale indices out of bounds: start={start}, end={end}, scales.length={len(scales)}")
    for i in range(start, end):
        if scales[i] <= 0:
            raise InvalidArgumentException("Scale values must be positive for logarithmic integration. "
                                           f"Found non-positive scale at index {i}: {_jd(scales[i])}")
    if n == 1:
        return [float(scales[start])]
    weights = [0.0] * n
    for i in range(n):
        if i == 0:
            weights[i] = math.log(scales[start + 1] / scales[start]) / 2.0
        elif i == n - 1:
            weights[i] = math.log(scales[start + i] / scales[start + i - 1]) / 2.0
        else:
            weights[i] = math.log(scales[start + i + 1] / scales[start + i - 1]) / 2.0
    return weights


def admissibility_numerical(wavelet: ContinuousWavelet) -> float:
    """InverseCWT.calculateAdmissibilityNumerical / waveletFourierTransform (:490-538): every frequency's sums run
    over t in the reference's order (one numpy operation per t over all frequencies), the outer sum in its order."""
    nPoints, maxFreq = 10000, 100.0
    freqs = np.zeros(nPoints)
    for i in range(1, nPoints):
        freqs[i] = maxFreq * math.pow(10.0, -4.0 + 4.0 * i / (nPoints - 1))
    omega = freqs[1:nPoints - 1]
    nT, tMax = 1000, 20.0
    dt = 2.0 * tMax / nT
    realSum = np.zeros_like(omega)
    imagSum = np.zeros_like(omega)
    for i in range(nT):
        t = -tMax + i * dt
        psi = wavelet.psi(t)
        arg = -omega * t
        realSum = realSum + psi * np.cos(arg) * dt
        imagSum = imagSum + psi * np.sin(arg) * dt
    psiHat = np.sqrt(realSum * realSum + imagSum * imagSum)
    integrand = psiHat * psiHat / omega
    total = 0.0
    for i in range(1, nPoints - 1):
        dOmega = (freqs[i + 1] - freqs[i - 1]) / 2.0
        total += float(integrand[i - 1]) * dOmega
    return float(2.0 * math.pi * total)


def admissibility_constant(wavelet: ContinuousWavelet) -> float:
    """InverseCWT.calculateAdmissibilityConstant (:462-485): by name, else numerically (cached on the wavelet)."""
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
    cached = getattr(wavelet, "_admissibility_numerical", None)
    if cached is None:
        cached = admissibility_numerical(wavelet)
        try:
            wavelet._admissibility_numerical = cached
        except AttributeError:  # pragma: no cover  (a wavelet class with __slots__)
            pass
    return cached


@dataclass
class ICWTTables:
    """What one vw_icwt_* call takes, for a wavelet, the scales [start, end) of a result and a row length."""
    form: int                                               # nat.ICWT_SUM or nat.ICWT_DIRECT
    scales: List[Tuple[int, int, int, int, float, float]]   # (tap_begin, taps, window_begin, plane, weight, scale)
    taps: np.ndarray                                        # float64, flat
    wrap: int                                               # M of ICWT_SUM (0 otherwise)
    divisor: float                                          # C_psi


def inverse_kernel_row(wavelet: ContinuousWavelet, scale: float, M: int) -> Tuple[int, List[float]]:
    """createWaveletFFT's time-domain table (:561-586) as g(d) = psi(d / scale) / sqrt(scale) over d in (-M/2, M/2]
    (index i <= M/2: d = i, else d = i - M).  -> (d_min, [g(d_min) .. g(M/2)])."""
    d_min = -(M // 2) + 1 if M > 1 else 0
    sqrtScale = math.sqrt(scale)
    return d_min, [wavelet.psi(d / scale) / sqrtScale for d in range(d_min, M // 2 + 1)]


def build_inverse_tables(wavelet: ContinuousWavelet, scales: Sequence[float], N: int, start: int, end: int,
                         trim: bool = True) -> ICWTTables:
    """The table and descriptors of InverseCWT.reconstructInternalReal(planes, scales, N, start, end): the route as
    :213.  trim=False keeps every entry of a SUM table (tests: trimming changes no bit)."""
    weights = log_scale_weights(scales, start, end)
    c_psi = admissibility_constant(wavelet)
    desc, taps = [], []
    if N >= ICWT_FFT_MIN_LENGTH:
        M = next_power_of_two(N)
        for j in range(start, end):
            a = scales[j]
            d_min, g = inverse_kernel_row(wavelet, a, M)
            lo, hi = 0, len(g) - 1
            if trim:   # an entry that is exactly 0.0 adds nothing to a finite sum
                while hi > lo and g[hi] == 0.0:
                    hi -= 1
                while lo < hi and g[lo] == 0.0:
                    lo += 1
            d_max = d_min + hi
            begin = len(taps)
            taps.extend(g[i] for i in range(hi, lo - 1, -1))   # w[k] = g(d_max - k)
            desc.append((begin, hi - lo + 1, -d_max, j, weights[j - start] / a, a))
        return ICWTTables(nat.ICWT_SUM, desc, np.asarray(taps, dtype=np.float64), M, c_psi)
    for j in range(start, end):   # reconstructionKernel (:359-374): (1.0 / sqrt(a)) * psi((t - b) / a)
        a = scales[j]
        scaleFactor = 1.0 / math.sqrt(a)
        begin = len(taps)
        taps.extend(scaleFactor * wavelet.psi(d / a) for d in range(-(N - 1), N))
        desc.append((begin, 2 * N - 1, 0, j, weights[j - start], a))
    return ICWTTables(nat.ICWT_DIRECT, desc, np.asarray(taps, dtype=np.float64), 0, c_psi)


class InverseCWT:
    """cwt/InverseCWT.java over a CWTResult holding planes [S, N] (one signal) or [B, S, N] (a batch), numpy (host
    memory) or CUDA tensors (device memory), float64 or float32 -> [N] / [B, N] in the same memory.  fma=True: one
    fma per term of the N >= 128 route instead of separate multiplies and adds (the N < 128 route divides every term:
    the flag is dropped there)."""

    def __init__(self, wavelet: ContinuousWavelet, fma: bool = False, engine: Optional[Engine] = None):
        if wavelet is None:
            raise InvalidArgumentException("Wavelet cannot be null")
        self.wavelet = wavelet
        self.admissibilityConstant = admissibility_constant(wavelet)
        if self.admissibilityConstant <= 0 or math.isinf(self.admissibilityConstant):
            raise InvalidConfigurationException(
                "Wavelet does not satisfy admissibility condition: C_ψ = " + _jd(self.admissibilityConstant))
        self.fma = bool(fma)
        self._engine = engine
        self._tables = {}

    def getAdmissibilityConstant(self) -> float:
        return self.admissibilityConstant

    def isAdmissible(self) -> bool:
        return self.admissibilityConstant > 0 and self.admissibilityConstant < math.inf

    def tables(self, scales: Sequence[float], N: int, start: int, end: int) -> ICWTTables:
        key = (tuple(scales), N, start, end)
        t = self._tables.get(key)
        if t is None:
            self._tables.clear()   # one shape at a time, as CWTTransform.tables
            t = self._tables[key] = build_inverse_tables(self.wavelet, scales, N, start, end)
        return t

    def reconstruct(self, cwtResult: CWTResult):
        if cwtResult is None:
            raise InvalidArgumentException("CWT result cannot be null")
        scales = cwtResult.getScales()
        if scales is None or len(scales) == 0:
            raise InvalidArgumentException("CWT result has no scales")
        coeffs = cwtResult.getCoefficients()
        signalLength = cwtResult.getNumSamples() if coeffs is not None else 0
        if coeffs is not None and signalLength <= 0:
            raise InvalidArgumentException(f"Invalid signal length: {signalLength}")
        if coeffs is None or coeffs.shape[-2] == 0:
            raise InvalidArgumentException("CWT result has no coefficients")
        return self._reconstruct(coeffs, scales, signalLength, 0, len(scales))

    def reconstructBand(self, cwtResult: CWTResult, minScale: float, maxScale: float):
        if cwtResult is None:
            raise InvalidArgumentException("CWT result cannot be null")
        if minScale <= 0 or maxScale <= minScale:
            raise InvalidArgumentException(f"Invalid scale range: minScale={_jd(minScale)}, maxScale={_jd(maxScale)}")
        scales = cwtResult.getScales()
        signalLength = cwtResult.getNumSamples()
        startIdx = endIdx = -1
        for i, s in enumerate(scales):
            if startIdx == -1 and s >= minScale:
                startIdx = i
            if s > maxScale:
                endIdx = i
                break
        if startIdx == -1:
            startIdx = 0
        if endIdx == -1:
            endIdx = len(scales)
        coeffs = cwtResult.getCoefficients()
        if startIdx >= endIdx:   # no scale in the requested range: the zero signal (:164-167)
            shape = tuple(coeffs.shape[:-2]) + (signalLength,)
            if _is_tensor(coeffs):
                return torch.zeros(shape, dtype=coeffs.dtype, device=coeffs.device)
            return np.zeros(shape, dtype=np.float32 if coeffs.dtype == np.float32 else np.float64)
        return self._reconstruct(coeffs, scales, signalLength, startIdx, endIdx)

    def reconstructFrequencyBand(self, cwtResult: CWTResult, samplingRate: float, minFreq: float, maxFreq: float):
        if samplingRate <= 0:
            raise InvalidArgumentException("Sampling rate must be positive")
        if minFreq < 0 or maxFreq <= minFreq or maxFreq > samplingRate / 2:
            raise InvalidArgumentException(f"Invalid frequency range: minFreq={_jd(minFreq)}, maxFreq={_jd(maxFreq)}")
        centerFreq = self.wavelet.centerFrequency()
        maxScale = centerFreq * samplingRate / minFreq if minFreq != 0 else math.copysign(math.inf, centerFreq * samplingRate)
        minScale = centerFreq * samplingRate / maxFreq
        return self.reconstructBand(cwtResult, minScale, maxScale)

    def _reconstruct(self, coeffs, scales, N: int, start: int, end: int):
        if len(coeffs.shape) not in (2, 3):
            raise InvalidArgumentException("Coefficients must be [S, N] or [B, S, N]")
        eng = self._engine
        if eng is None:
            dev = coeffs.device.index if (_is_tensor(coeffs) and coeffs.is_cuda) else None
            eng = Engine.get(dev)
        t = self.tables(scales, N, start, end)
        flags = nat.FLAG_FMA if (self.fma and t.form == nat.ICWT_SUM) else 0
        return eng.icwt(coeffs, t.scales, t.taps, t.form, t.wrap, t.divisor, flags)
