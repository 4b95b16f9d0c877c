"""vectorwave_amd -- MI355X (gfx950) MODWT / SWT engine with VectorWave's API.

The compute path is libvectorwave_amd.so (hand-written HIP kernels behind a C ABI,
include/vectorwave_amd.h).  This package is the host-side mirror of the reference's Java API:

  MODWTTransform, MultiLevelMODWTTransform, MODWTResult, MultiLevelMODWTResult,
  MutableMultiLevelMODWTResult, BoundaryMode                  (core/modwt, core/api)
  VectorWaveSwtAdapter                                        (core/swt)
  WaveletDenoiser                                             (core/denoising)
  FinancialAnalyzer, FinancialWaveletAnalyzer and their configs (com.morphiqlabs.financial)
  MODWTStreamingTransform, MultiLevelMODWTStreamingTransform  (core/modwt/streaming)
  BatchMODWT, BatchStreamingMODWT                             (ext/extensions/modwt)
  Haar, Daubechies, Symlet, Coiflet, BiorthogonalSpline,
  ReverseBiorthogonalSpline                                   (core/api wavelets)
  CWTTransform, CWTConfig, CWTResult, ScaleSpace, MorletWavelet,
  RickerWavelet, PaulWavelet, DOGWavelet, InverseCWT          (core/cwt, core/cwt/finance)
"""
from .wavelets import (BiorthogonalSpline, BiorthogonalWavelet, Coiflet, Daubechies, Haar, ReverseBiorthogonalSpline,
                       Symlet, Wavelet, available_wavelets, get_wavelet)
from .errors import (ErrorCode, InvalidArgumentException, InvalidConfigurationException, InvalidSignalException,
                     InvalidStateException, WaveletTransformException)
from .modwt import (BoundaryMode, MODWTResult, MODWTTransform, MultiLevelMODWTResult, MultiLevelMODWTTransform,
                    MutableMultiLevelMODWTResult)
from .swt import VectorWaveSwtAdapter
from .denoise import ThresholdMethod, ThresholdType, WaveletDenoiser
from .streaming import (MODWTStreamingDenoiser, MODWTStreamingTransform, MODWTStreamingTransformImpl,
                        MultiLevelMODWTStreamingTransform)
from .batch import BatchMODWT, BatchSIMDMODWT, BatchStreamingMODWT
from .financial import (FinancialAnalysisConfig, FinancialAnalyzer, FinancialConfig, FinancialWaveletAnalyzer,
                        VolatilityClassification)
from .engine import Engine, max_levels, version
from .multidevice import DeviceGroup
from .cwt import (ComplexContinuousWavelet, ContinuousWavelet, CWTConfig, CWTResult, CWTTransform, DOGWavelet,
                  InverseCWT, MorletWavelet, PaddingStrategy, PaulWavelet, RickerWavelet, ScaleSpace)

__all__ = [
    "Coiflet", "Daubechies", "Haar", "Symlet", "Wavelet", "available_wavelets", "get_wavelet",
    "ErrorCode", "InvalidArgumentException", "InvalidSignalException", "InvalidStateException",
    "WaveletTransformException", "BoundaryMode", "MODWTResult", "MODWTTransform", "MultiLevelMODWTResult",
    "MultiLevelMODWTTransform", "MutableMultiLevelMODWTResult", "VectorWaveSwtAdapter", "BatchMODWT",
    "WaveletDenoiser", "ThresholdMethod", "ThresholdType", "BatchSIMDMODWT", "MODWTStreamingTransform",
    "MODWTStreamingTransformImpl", "MultiLevelMODWTStreamingTransform",
    "BatchStreamingMODWT", "Engine", "max_levels", "version", "DeviceGroup",
    "FinancialAnalysisConfig", "FinancialAnalyzer", "FinancialConfig", "FinancialWaveletAnalyzer",
    "VolatilityClassification", "BiorthogonalSpline", "BiorthogonalWavelet", "ReverseBiorthogonalSpline",
    "ComplexContinuousWavelet", "ContinuousWavelet", "CWTConfig", "CWTResult", "CWTTransform", "DOGWavelet",
    "MorletWavelet", "PaddingStrategy", "PaulWavelet", "RickerWavelet", "ScaleSpace", "InverseCWT",
    "InvalidConfigurationException",
]
