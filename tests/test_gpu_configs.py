"""GPU parity at the BASELINE.json config shapes themselves (through the C ABI, vs the CPU restatement).

  config 1  Haar MODWT level-1 PERIODIC, N = 1024                 MODWTTransform.java:131-299
  config 3  sym8 SWT J=8 + universal soft-threshold denoise, N = 16384
            (VectorWaveSwtAdapter.denoise :546-574: forward -> sigma = MAD(d_1)/0.6745 ->
             T = sigma*sqrt(2 ln N) soft on every detail level -> reconstructPeriodic)
  config 4  db8 MODWT J=10 on a 2^20-sample PERIODIC block, BatchMODWT semantics (no level cap,
            BatchMODWT.java:90-111 / BatchSIMDMODWT.java:343-424; inverse = core reconstruct per signal,
            BatchMODWT.java:151-178) -- exercises k_forward_multi, the column sweeps and k_inverse_multi
  config 5  coif5 MODWT J=6 fp32, N = 8192 (no fp32 path in the reference: compared with the fp64
            restatement at a relative tolerance)

Bar: bit-exact (max-abs 0) in EXACT mode, thresholds equal; FMA within 1e-12 * max|x| (north_star) and, for the
config 4 and config 5 transforms, bit-exact against the restatement's FMA form on the rows picked
(tests/restatement_generic.py ``fma=True``; the denoise chain of config 3 keeps its tolerance).
"""
import math

import numpy as np
import pytest

from oracle import oracle as O
import vectorwave_amd as vw
from vectorwave_amd.wavelets import Coiflet, Daubechies, Haar, Symlet

import restatement_generic as G

pytestmark = pytest.mark.gpu


def lohi(w):
    return w.lowPassDecomposition(), w.highPassDecomposition()


def exact(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    if not np.array_equal(a, b):
        i = np.unravel_index(np.argmax(np.abs(a - b)), a.shape)
        raise AssertionError(f"{what} not bit-exact: max |diff| = {np.max(np.abs(a - b)):.3e} at {i}")


def config3_signals(B, n, seed=42):
    """SURVEY.md §8d config 3 input: sin(2pi 3i/N) + 0.5 sin(2pi 37i/N) + 0.2 z, z Box-Muller of counter u."""
    i = np.arange(n)
    base = np.sin(2 * np.pi * 3 * i / n) + 0.5 * np.sin(2 * np.pi * 37 * i / n)
    out = np.empty((B, n))
    for b in range(B):
        u1 = O.fill_uniform(n, seed, offset=(2 * b) * n) * 0.5 + 0.5      # (x+1)/2 in [0,1)
        u2 = O.fill_uniform(n, seed, offset=(2 * b + 1) * n) * 0.5 + 0.5
        z = np.sqrt(-2.0 * np.log1p(-u1)) * np.cos(2 * np.pi * u2)
        out[b] = base + 0.2 * z
    return out


def test_config1_haar_level1_n1024(engine):
    w = Haar.INSTANCE
    x = O.fill_uniform(1024, 42)
    tx = vw.MODWTTransform(w, vw.BoundaryMode.PERIODIC)
    r = tx.forward(x)
    a_ref, d_ref = O.modwt_forward(x, *lohi(w), O.PERIODIC)
    exact(r.approximationCoeffs(), a_ref, "approx")
    exact(r.detailCoeffs(), d_ref, "detail")
    y = tx.inverse(r)
    exact(y, O.modwt_inverse(a_ref, d_ref, w.lowPassReconstruction(), w.highPassReconstruction(), O.PERIODIC), "y")
    # the reference's own known answer (MODWTPercivalWaldenValidationTest.java:73)
    r4 = tx.forward(np.array([1.0, 2.0, 3.0, 4.0]))
    np.testing.assert_allclose(r4.approximationCoeffs(), [2.5, 1.5, 2.5, 3.5], rtol=0, atol=1e-12)


@pytest.mark.parametrize("fma", [False, True], ids=["exact", "fma"])
def test_config3_sym8_swt_j8_denoise_16384(engine, fma):
    w = Symlet.SYM8
    n, J, B = 16384, 8, 4
    x = config3_signals(B, n)
    swt = vw.VectorWaveSwtAdapter(w, vw.BoundaryMode.PERIODIC, fma=fma)
    y, thr = swt.denoise(x, J, return_thresholds=True)   # threshold < 0: universal, soft
    for b in range(B):
        y_ref, t_ref = O.swt_denoise(x[b], *lohi(w), O.PERIODIC, J, -1.0, True, wavelet_id=w.wavelet_id)
        if fma:
            assert abs(thr[b] - t_ref) <= 1e-12 * abs(t_ref)
            np.testing.assert_allclose(y[b], y_ref, rtol=0, atol=1e-12 * np.max(np.abs(x[b])))
        else:
            assert thr[b] == t_ref, (b, thr[b], t_ref)
            exact(y[b], y_ref, f"denoised signal {b}")


def test_config3_device_tensors_batch(engine):
    # the same pipeline on device-resident tensors (the bench path), 8 signals, EXACT
    import torch
    w = Symlet.SYM8
    n, J, B = 16384, 8, 8
    x = config3_signals(B, n, seed=7)
    xd = torch.from_numpy(x).cuda()
    y, thr = vw.VectorWaveSwtAdapter(w, vw.BoundaryMode.PERIODIC).denoise(xd, J, return_thresholds=True)
    y, thr = y.cpu().numpy(), thr.cpu().numpy()
    for b in (0, 5, 7):
        y_ref, t_ref = O.swt_denoise(x[b], *lohi(w), O.PERIODIC, J, wavelet_id=w.wavelet_id)
        assert thr[b] == t_ref
        exact(y[b], y_ref, f"signal {b}")


def test_config4_db8_j10_block_2p20(engine):
    w = Daubechies.DB8
    n, J = 1 << 20, 10
    x = O.fill_uniform(n, 42).reshape(1, n)
    m = vw.BatchMODWT.multiLevelAoS(w, x, J)
    d_ref, a_ref = O.decompose(x[0], *lohi(w), O.PERIODIC, J, core=False)
    for j in range(J):
        exact(m.detailPerLevel[j, 0], d_ref[j], f"detail level {j + 1}")
    exact(m.finalApprox[0], a_ref, "approximation")
    y = vw.BatchMODWT.inverseMultiLevelAoS(w, m.detailPerLevel, m.finalApprox)
    y_ref = O.reconstruct(d_ref, a_ref, w.lowPassReconstruction(), w.highPassReconstruction(), O.PERIODIC,
                          w.wavelet_id)
    exact(y[0], y_ref, "inverse")
    # FMA mode on the same block: within the north_star tolerance of the exact result
    mf = vw.BatchMODWT.multiLevelAoS(w, x, J, fma=True)
    for j in range(J):
        np.testing.assert_allclose(mf.detailPerLevel[j, 0], d_ref[j], rtol=0, atol=1e-12)
    yf = vw.BatchMODWT.inverseMultiLevelAoS(w, mf.detailPerLevel, mf.finalApprox, fma=True)
    np.testing.assert_allclose(yf[0], y_ref, rtol=0, atol=1e-12)


def test_config4_streaming_blocks_independent(engine):
    # BatchStreamingMODWT PERIODIC: every 2^20 block is an independent transform (BatchStreamingMODWT
    # .java:110-116); two blocks of a 2-signal batch, second block compared level by level
    import torch
    w = Daubechies.DB8
    n, J = 1 << 20, 10
    s = vw.BatchStreamingMODWT(w, vw.BoundaryMode.PERIODIC, J)
    blocks = [O.fill_uniform(2 * n, 42, offset=k * 2 * n).reshape(2, n) for k in range(2)]
    for k, blk in enumerate(blocks):
        r = s.processMultiLevel(torch.from_numpy(blk).cuda())
    det = r.detailPerLevel.cpu().numpy()
    for b in (1,):
        d_ref, a_ref = O.decompose(blocks[1][b], *lohi(w), O.PERIODIC, J, core=False)
        exact(det[:, b, :], d_ref, "block 2 details")
        exact(r.finalApprox[b].cpu().numpy(), a_ref, "block 2 approximation")


def test_config5_coif5_f32_j6_8192(engine):
    import torch
    w = Coiflet.COIF5
    n, J, B = 8192, 6, 64
    x64 = O.fill_uniform(B * n, 42).reshape(B, n)
    x32 = x64.astype(np.float32)
    xd = torch.from_numpy(x32).cuda()
    tx = vw.MultiLevelMODWTTransform(w, vw.BoundaryMode.PERIODIC, fma=True)
    res = tx.decompose(xd, J)
    y = tx.reconstruct(res).cpu().numpy()
    det, app = res.details_array.cpu().numpy(), res.approximation_array.cpu().numpy()
    assert det.dtype == np.float32 and y.dtype == np.float32
    # SURVEY.md §8d fp32 bar: 1e-5 * max|x| * J (fp32 rounding through J levels of 30-tap sums)
    tol = 1e-5 * float(np.max(np.abs(x32))) * J
    # FMA bits: the float32 FMA restatement (fmaf(x, f, acc) per tap) of the rows picked below, in one pass
    rows = list(range(0, B, 9))
    d_fma, a_fma = G.decompose(x32[rows], *lohi(w), O.PERIODIC, J, dtype=np.float32, fma=True)
    y_fma = G.reconstruct(d_fma, a_fma, w.lowPassReconstruction(), w.highPassReconstruction(), O.PERIODIC, w.wavelet_id,
                          dtype=np.float32, fma=True)
    exact(det[:, rows, :], d_fma, "FMA details")
    exact(app[rows], a_fma, "FMA approximation")
    exact(y[rows], y_fma, "FMA inverse")
    for b in range(0, B, 9):
        xr = x32[b].astype(np.float64)
        d_ref, a_ref = O.decompose(xr, *lohi(w), O.PERIODIC, J)
        np.testing.assert_allclose(det[:, b, :], d_ref, rtol=0, atol=tol)
        np.testing.assert_allclose(app[b], a_ref, rtol=0, atol=tol)
        y_ref = O.reconstruct(d_ref, a_ref, w.lowPassReconstruction(), w.highPassReconstruction(), O.PERIODIC)
        np.testing.assert_allclose(y[b], y_ref, rtol=0, atol=tol)
    assert np.max(np.abs(y - x32)) < 1e-3  # coif5's truncated taps + fp32


# ---- full BASELINE batch sizes: the kernel policy sees the real batch, so a policy that
# switches with B (two-buffer inverse at small batches, NV = 2, persistent grids) is exercised exactly as
# bench.py runs it.  Inputs as bench.py's (counter-based uniform, generated on device), C-ABI calls on
# device buffers; first / middle / last rows against the restatement.
def _full_rows(B):
    return (0, B // 2 - 1, B - 1)


@pytest.mark.parametrize("fma", [False, True], ids=["exact", "fma"])
def test_config3_full_batch_16384x16384(engine, fma):
    import torch
    from ctypes import c_void_p
    from vectorwave_amd import _native as nat
    w = Symlet.SYM8
    n, J, B = 16384, 8, 16384
    x = torch.empty((B, n), dtype=torch.float64, device="cuda")
    engine.fill_uniform(x, 42)
    y = torch.empty_like(x)
    thr = torch.empty((B,), dtype=torch.float64, device="cuda")
    lo, hi = lohi(w)
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    engine.bind_torch_stream()
    st = engine.lib.vw_swt_denoise_f64(engine.ctx, P(x), B, n, n, nat.taps_array(lo), nat.taps_array(hi), len(lo),
                                       w.wavelet_id, nat.PERIODIC, J, -1.0, 1, nat.FLAG_FMA if fma else 0, P(y),
                                       P(thr))
    assert st == 0, nat.last_error()
    torch.cuda.synchronize()
    for b in _full_rows(B):
        xr = x[b].cpu().numpy()
        y_ref, t_ref = O.swt_denoise(xr, lo, hi, O.PERIODIC, J, -1.0, True, wavelet_id=w.wavelet_id)
        if fma:
            assert abs(thr[b].item() - t_ref) <= 1e-12 * abs(t_ref)
            np.testing.assert_allclose(y[b].cpu().numpy(), y_ref, rtol=0, atol=1e-12 * np.max(np.abs(xr)))
        else:
            assert thr[b].item() == t_ref
            exact(y[b].cpu().numpy(), y_ref, f"denoised signal {b}")
    del x, y


@pytest.mark.parametrize("fma", [False, True], ids=["exact", "fma"])
def test_config4_full_batch_256x2p20(engine, fma):
    # VERDICT r4 next #1a: the bench's db8-stream batch itself (256 PERIODIC blocks of 2^20 samples, J = 10,
    # BatchMODWT semantics).  The deep forward cuts each signal into segments so the grid fills the GPU and
    # the inverse's chained sweeps / multi-level tiles plan by B, so the 256-row plan bench.py times is
    # pinned here, not a B = 1 / 2 stand-in.  Same C-ABI calls as bench.py Part.step_fn, device-generated
    # input (seed 42, offset 0), rows 0 / 127 / 255 vs BatchMODWT.multiLevelAoS + core reconstruct
    # (BatchMODWT.java:90-111,151-178).
    import torch
    from ctypes import c_void_p
    from vectorwave_amd import _native as nat
    w = Daubechies.DB8
    n, J, B = 1 << 20, 10, 256
    x = torch.empty((B, n), dtype=torch.float64, device="cuda")
    engine.fill_uniform(x, 42)
    det = torch.empty((J, B, n), dtype=torch.float64, device="cuda")
    app = torch.empty_like(x)
    y = torch.empty_like(x)
    lo, hi = lohi(w)
    la, ha = nat.taps_array(lo), nat.taps_array(hi)
    flags = nat.FLAG_FMA if fma else 0
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    engine.bind_torch_stream()
    lib = engine.lib
    assert lib.vw_modwt_forward_f64(engine.ctx, P(x), B, n, n, la, ha, len(lo), w.wavelet_id, nat.PERIODIC, J,
                                    flags, P(det), P(app)) == 0, nat.last_error()
    assert lib.vw_modwt_inverse_f64(engine.ctx, P(det), P(app), B, n, la, ha, len(lo), w.wavelet_id, nat.PERIODIC,
                                    J, 0xFFFFFFFF, 0, flags, P(y)) == 0, nat.last_error()
    torch.cuda.synchronize()
    if fma:   # FMA bits: the restatement's fma(x, f, acc) chain on the three rows picked below, in one pass
        rows = [0, B // 2 - 1, B - 1]
        d_fma, a_fma = G.decompose(x[rows].cpu().numpy(), lo, hi, O.PERIODIC, J, fma=True)
        y_fma = G.reconstruct(d_fma, a_fma, w.lowPassReconstruction(), w.highPassReconstruction(), O.PERIODIC,
                              w.wavelet_id, fma=True)
        exact(det[:, rows, :].cpu().numpy(), d_fma, "FMA details")
        exact(app[rows].cpu().numpy(), a_fma, "FMA approximation")
        exact(y[rows].cpu().numpy(), y_fma, "FMA inverse")
        del d_fma, a_fma, y_fma
    for b in (0, B // 2 - 1, B - 1):
        xr = x[b].cpu().numpy()
        d_ref, a_ref = O.decompose(xr, lo, hi, O.PERIODIC, J, core=False)
        y_ref = O.reconstruct(d_ref, a_ref, w.lowPassReconstruction(), w.highPassReconstruction(), O.PERIODIC,
                              w.wavelet_id)
        got_d, got_a, got_y = det[:, b, :].cpu().numpy(), app[b].cpu().numpy(), y[b].cpu().numpy()
        if fma:
            np.testing.assert_allclose(got_d, d_ref, rtol=0, atol=1e-12)
            np.testing.assert_allclose(got_a, a_ref, rtol=0, atol=1e-12)
            np.testing.assert_allclose(got_y, y_ref, rtol=0, atol=1e-12)
        else:
            exact(got_d, d_ref, f"signal {b} details")
            exact(got_a, a_ref, f"signal {b} approximation")
            exact(got_y, y_ref, f"signal {b} inverse")
    # every row: perfect reconstruction within db8's truncated published taps (bench.py verify bar)
    assert float((y - x).abs().max().item()) < 1e-8
    del x, det, app, y


def test_config5_full_batch_65536x8192_f32(engine):
    import torch
    from ctypes import c_void_p
    from vectorwave_amd import _native as nat
    w = Coiflet.COIF5
    n, J, B = 8192, 6, 65536
    x = torch.empty((B, n), dtype=torch.float32, device="cuda")
    engine.fill_uniform(x, 42)
    det = torch.empty((J, B, n), dtype=torch.float32, device="cuda")
    app = torch.empty_like(x)
    y = torch.empty_like(x)
    lo, hi = lohi(w)
    la, ha = nat.taps_array(lo), nat.taps_array(hi)
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    engine.bind_torch_stream()
    lib = engine.lib
    assert lib.vw_modwt_forward_f32(engine.ctx, P(x), B, n, n, la, ha, len(lo), w.wavelet_id, nat.PERIODIC, J,
                                    nat.FLAG_FMA, P(det), P(app)) == 0, nat.last_error()
    assert lib.vw_modwt_inverse_f32(engine.ctx, P(det), P(app), B, n, la, ha, len(lo), w.wavelet_id, nat.PERIODIC,
                                    J, 0xFFFFFFFF, 0, nat.FLAG_FMA, P(y)) == 0, nat.last_error()
    torch.cuda.synchronize()
    rows = list(_full_rows(B))   # FMA bits: the float32 FMA restatement of the rows picked below
    d_fma, a_fma = G.decompose(x[rows].cpu().numpy(), lo, hi, O.PERIODIC, J, dtype=np.float32, fma=True)
    y_fma = G.reconstruct(d_fma, a_fma, w.lowPassReconstruction(), w.highPassReconstruction(), O.PERIODIC, w.wavelet_id,
                          dtype=np.float32, fma=True)
    exact(det[:, rows, :].cpu().numpy(), d_fma, "FMA details")
    exact(app[rows].cpu().numpy(), a_fma, "FMA approximation")
    exact(y[rows].cpu().numpy(), y_fma, "FMA inverse")
    for b in _full_rows(B):
        xr = x[b].double().cpu().numpy()
        tol = 1e-5 * float(np.max(np.abs(xr))) * J
        d_ref, a_ref = O.decompose(xr, lo, hi, O.PERIODIC, J)
        y_ref = O.reconstruct(d_ref, a_ref, w.lowPassReconstruction(), w.highPassReconstruction(), O.PERIODIC)
        np.testing.assert_allclose(det[:, b, :].double().cpu().numpy(), d_ref, rtol=0, atol=tol)
        np.testing.assert_allclose(app[b].double().cpu().numpy(), a_ref, rtol=0, atol=tol)
        np.testing.assert_allclose(y[b].double().cpu().numpy(), y_ref, rtol=0, atol=tol)
    del x, det, app, y
