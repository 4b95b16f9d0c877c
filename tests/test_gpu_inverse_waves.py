"""VW_INV_WAVES: the PLAIN form of the one-buffer inverse k_inverse_seq at 6 and at 8 waves per SIMD.

A full-slab PERIODIC fp64 reconstruction of a short filter (L <= 8) from all of its coefficient planes runs
inverse_seq_plain (vw_dev_inv.h), compiled for 6 waves per SIMD (three 512-thread workgroups per CU) and for 8
(64 VGPRs: four).  Only registers, addresses and the number of LDS reads in flight differ between the two and
from the general kernel: per output the taps, their order and the multiply/add instructions are the same, so y is
bit-identical under both settings, EXACT is bit-exact against the restatement and FMA within 1e-12 of it
(tests/test_gpu_parity.py's bars).  Everything the PLAIN form leaves out -- thresholds, SYMMETRIC shifts, ragged
slabs -- keeps the general kernels whatever the switch says, with the results tests/test_gpu_level_strides.py
asserts for them.
"""
import numpy as np
import pytest

from oracle import oracle as O
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import Daubechies, Haar, Symlet

pytestmark = pytest.mark.gpu

# 2, 4, 6 and 8 taps (sym3: the catalogue's six-tap Daubechies-3)
WAVELETS = [Haar.INSTANCE, Daubechies.DB2, Symlet.SYM3, Daubechies.DB4]
# N = 512, J = 6: the smallest full-slab shape (64 threads x 4 vectors), spacings 1..32, the deep levels' halos
# wider than the first slab (copied after a barrier); N = 1024, J = 7 adds spacing 64
SHAPES = [(512, 6), (1024, 7)]


def lohi(w):
    return w.lowPassDecomposition(), w.highPassDecomposition()


def rlohi(w):
    return w.lowPassReconstruction(), w.highPassReconstruction()


def coefficients(engine, x, w, J, flags):
    import torch
    det, app = engine.forward(x, *lohi(w), w.wavelet_id, O.PERIODIC, J, flags)
    torch.cuda.synchronize()
    return det, app


def inverse(engine, det, app, w, J, flags, waves):
    import torch
    with engine.options(VW_INV_WAVES=waves, VW_INV_BUF=1):  # the one-buffer kernel at small batches too
        y = engine.inverse(det, app, *rlohi(w), w.wavelet_id, O.PERIODIC, J, flags)
        torch.cuda.synchronize()
    return y


def check(engine, x, w, J, rows):
    """EXACT and FMA: y at 8 waves == y at 6 waves bit for bit; rows against the restatement."""
    import torch
    for flags in (0, nat.FLAG_FMA):
        det, app = coefficients(engine, x, w, J, flags)
        y6 = inverse(engine, det, app, w, J, flags, 6)
        y8 = inverse(engine, det, app, w, J, flags, 8)
        assert torch.equal(y8, y6), f"flags={flags}: VW_INV_WAVES=8 differs from VW_INV_WAVES=6"
        for b in rows:
            d_ref, a_ref = O.decompose(x[b].cpu().numpy(), *lohi(w), O.PERIODIC, J, core=False)
            y_ref = O.reconstruct(d_ref, a_ref, *rlohi(w), O.PERIODIC, w.wavelet_id)
            got = y8[b].cpu().numpy()
            err = float(np.max(np.abs(got - y_ref)))
            print(f"  flags={flags} row {b}: max|y - ref| = {err:.3e}")
            if flags & nat.FLAG_FMA:
                assert err <= 1e-12, f"row {b}: {err:.3e} > 1e-12"
            else:
                assert np.array_equal(got, y_ref), f"row {b} not bit-exact ({err:.3e})"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}-J{s[1]}")
@pytest.mark.parametrize("w", WAVELETS, ids=lambda w: w.name())
def test_eight_waves_match_six_and_the_restatement(engine, w, shape):
    import torch
    n, J = shape
    x = torch.empty((5, n), dtype=torch.float64, device="cuda")
    engine.fill_uniform(x, 211)
    check(engine, x, w, J, (0, 2, 4))


def test_headline_workgroup_shape(engine):
    """N = 4096: 512-thread workgroups, the register allocation the headline runs with; 9 rows."""
    import torch
    x = torch.empty((9, 4096), dtype=torch.float64, device="cuda")
    engine.fill_uniform(x, 213)
    check(engine, x, Daubechies.DB4, 6, (0, 4, 8))


def test_more_rows_than_resident_workgroups(engine):
    """32 one-wave workgroups per CU bound the resident set from above (32 waves per CU); + 3 rows: workgroup
    slots, their LDS and registers are reused by later rows."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 32 * cus + 3
    x = torch.empty((B, 512), dtype=torch.float64, device="cuda")
    engine.fill_uniform(x, 217)
    check(engine, x, Daubechies.DB4, 6, (0, B // 2, B - 1))


def signals(B, n, seed):
    return np.stack([O.java_random_signal(n, seed + b) for b in range(B)])


def test_ragged_rows_keep_the_checked_kernel(engine):
    """N = 500: the last slab is ragged, the plan is not full: no PLAIN form under either setting."""
    w, n, J = Daubechies.DB4, 500, 3
    x = signals(5, n, 47)
    for waves in (8, 6):
        with engine.options(VW_INV_WAVES=waves, VW_INV_BUF=1):
            det, app = engine.forward(x, *lohi(w), w.wavelet_id, O.PERIODIC, J, 0)
            y = engine.inverse(det, app, *rlohi(w), w.wavelet_id, O.PERIODIC, J, 0)
        for b in (0, 2, 4):
            d_ref, a_ref = O.decompose(x[b], *lohi(w), O.PERIODIC, J, core=False)
            assert np.array_equal(det[:, b, :], d_ref), f"details row {b} waves={waves}"
            assert np.array_equal(y[b], O.reconstruct(d_ref, a_ref, *rlohi(w), O.PERIODIC, w.wavelet_id)), \
                f"reconstruction row {b} waves={waves}"


def test_swt_denoise_thresholds_keep_the_general_kernel(engine):
    """Thresholds are applied on the general kernel's detail loads; the PLAIN form has no such path."""
    w, n, J = Daubechies.DB4, 512, 4
    x = signals(5, n, 43)
    swt = vw.VectorWaveSwtAdapter(w, vw.BoundaryMode.PERIODIC)
    ref = [O.swt_denoise(x[b], *lohi(w), O.PERIODIC, J, wavelet_id=w.wavelet_id) for b in range(5)]
    for waves in (8, 6):
        with engine.options(VW_INV_WAVES=waves, VW_INV_BUF=1):
            y, thr = swt.denoise(x, J, return_thresholds=True)
        for b in range(5):
            assert thr[b] == ref[b][1], f"threshold row {b} waves={waves}"
            assert np.array_equal(y[b], ref[b][0]), f"denoised row {b} waves={waves}"


def test_symmetric_reconstruct_keeps_the_general_kernel(engine):
    """SYMMETRIC: alignment shifts and both read directions; bit-exact under both settings."""
    w, n, J = Daubechies.DB4, 512, 4
    x = signals(5, n, 41)
    tx = vw.MultiLevelMODWTTransform(w, vw.BoundaryMode(O.SYMMETRIC))
    for waves in (8, 6):
        with engine.options(VW_INV_WAVES=waves, VW_INV_BUF=1):
            res = tx.decompose(x, J)
            y = tx.reconstruct(res)
        for b in (0, 2, 4):
            d_ref, a_ref = O.decompose(x[b], *lohi(w), O.SYMMETRIC, J)
            assert np.array_equal(res.details_array[:, b, :], d_ref), f"details row {b} waves={waves}"
            y_ref = O.reconstruct(d_ref, a_ref, *rlohi(w), O.SYMMETRIC, w.wavelet_id)
            assert np.array_equal(y[b], y_ref), f"reconstruction row {b} waves={waves}"
