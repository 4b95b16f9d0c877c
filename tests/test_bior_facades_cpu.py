"""The calls whose ABI takes ONE filter pair for both directions (denoise, streaming, energy, financial) refuse a
wavelet whose decomposition and reconstruction filters differ, with VW_ERR_UNSUPPORTED's exception type and a
message naming the wavelet, before any launch: none of these tests has a GPU to launch on."""
import numpy as np
import pytest

import vectorwave_amd as vw
from vectorwave_amd.wavelets import get_wavelet

W = get_wavelet("rbio4.4")
X = np.linspace(-1.0, 1.0, 2 * 128).reshape(2, 128)
refuses = pytest.raises(NotImplementedError, match=r"rbio4\.4")


def test_wavelet_denoiser():
    with refuses:
        vw.WaveletDenoiser(W, vw.BoundaryMode.PERIODIC)


def test_swt_denoise():
    with refuses:
        vw.VectorWaveSwtAdapter(W).denoise(X[0], 2)


def test_streaming():
    with refuses:
        vw.MODWTStreamingTransform.create(W, vw.BoundaryMode.PERIODIC, 64)
    with refuses:
        vw.MODWTStreamingTransform.createMultiLevel(W, vw.BoundaryMode.PERIODIC, 64, 2)
    with refuses:
        vw.BatchStreamingMODWT(W, vw.BoundaryMode.ZERO_PADDING, 2)
    with refuses:
        vw.BatchStreamingMODWT.builder().wavelet(W).levels(2).build()


def test_energy():
    with refuses:
        vw.BatchMODWT.energyBatch(W, X, 2)
    with refuses:
        vw.BatchMODWT.relativeEnergyBatch(W, X, 2)
    with refuses:
        vw.MultiLevelMODWTTransform(W, vw.BoundaryMode.PERIODIC).energyBatch(X, 2)


def test_financial():
    fa = vw.FinancialWaveletAnalyzer(vw.FinancialConfig(0.02), vw.MODWTTransform(W, vw.BoundaryMode.PERIODIC))
    with refuses:
        fa.calculateWaveletSharpeRatioBatch(X)


def test_batch_reach_guard_reads_the_low_pass_length():
    """BatchSIMDMODWT's loop is bounded by scaledLow.length for both filters (BatchSIMDMODWT.java:397), so the index
    that goes negative -- the reference's ArrayIndexOutOfBoundsException, IndexError here -- depends on the low-pass
    length alone: rbio1.5's analysis pair (2, 10) passes where its 10-tap high-pass would not, bior1.5's (10, 2)
    does not."""
    from vectorwave_amd.batch import _check_batch_reach
    n, levels = 64, 4                      # (10 - 1) * 8 + 1 = 73 > n + 1; (2 - 1) * 8 + 1 = 9
    _check_batch_reach(get_wavelet("rbio1.5"), n, levels)
    with pytest.raises(IndexError, match="level 4"):
        _check_batch_reach(get_wavelet("bior1.5"), n, levels)


def test_orthogonal_wavelets_are_not_refused():
    from vectorwave_amd.wavelets import require_orthogonal
    for name in ("haar", "db4", "sym8", "coif5", "bior1.1", "rbio1.1"):
        require_orthogonal(get_wavelet(name), "a single-pair path")
