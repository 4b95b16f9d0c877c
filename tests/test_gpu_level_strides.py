"""Compile-time level strides and full-slab forms of the fused short-filter kernels (VW_LEVEL_CT).

With VW_LEVEL_CT=1 (vw_dev_rows.h fwd_row_ct / inv_row_ct) a strided level of a tap-unrolled filter (L <= 8) is
dispatched once per row to a body with the spacing as a template constant (2..64; other spacings keep the
run-time body), and k_forward_persist / k_inverse_seq run without per-vector bounds checks where the host
contract makes every slab full.  Only addresses and control flow move: per output the taps, their order and
the multiply/add instructions are those of VW_LEVEL_CT=0, so every array is bit-identical between the two
settings in every mode, and EXACT is bit-exact against the restatement under both.

Bars against the restatement (tests/test_gpu_parity.py): EXACT fp64 bit-exact; FMA fp64 1e-12;
fp32 1e-5 * max|x| * J.
"""
import numpy as np
import pytest

from oracle import oracle as O
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import Daubechies, Haar, Symlet

pytestmark = pytest.mark.gpu

# 2, 4, 6 and 8 taps: haar, db2, db3 (the catalogue carries Daubechies-3 as sym3: the same six taps), db4
WAVELETS = [Haar.INSTANCE, Daubechies.DB2, Symlet.SYM3, Daubechies.DB4]
# (dtype, N, J): fp64 N = 512 is the persistent forward's smallest legal shape (64 threads x 4 vectors) and
# runs the spacings 2..32; N = 1024, J = 7 adds spacing 64; fp32 (V = 4): s = 2 is the register window,
# s >= 4 strided
SHAPES = [("f64", 512, 6), ("f64", 1024, 7), ("f32", 1024, 6)]
# kernel policies: the default (at 5 rows the two-buffer inverse k_inverse_db) and the one-buffer inverse
# k_inverse_seq that full batches run
POLICIES = [dict(), dict(VW_INV_BUF=1)]


def lohi(w):
    return w.lowPassDecomposition(), w.highPassDecomposition()


def rlohi(w):
    return w.lowPassReconstruction(), w.highPassReconstruction()


def fwd_inv(engine, x, w, boundary, J, flags, **opts):
    import torch
    with engine.options(**opts):
        det, app = engine.forward(x, *lohi(w), w.wavelet_id, boundary, J, flags)
        y = engine.inverse(det, app, *rlohi(w), w.wavelet_id, boundary, J, flags)
        torch.cuda.synchronize()
    return det, app, y


def check_rows(x, outs, w, J, flags, rows):
    """Rows of (det, app, y) against the restatement (BatchMODWT semantics: direct convolutions)."""
    det, app, y = outs
    f64 = x.dtype.itemsize == 8
    tol = 1e-12 if f64 else 1e-5 * float(x.abs().max().item()) * J
    for b in rows:
        d_ref, a_ref = O.decompose(x[b].double().cpu().numpy(), *lohi(w), O.PERIODIC, J, core=False)
        y_ref = O.reconstruct(d_ref, a_ref, *rlohi(w), O.PERIODIC, w.wavelet_id)
        got = (det[:, b, :].double().cpu().numpy(), app[b].double().cpu().numpy(), y[b].double().cpu().numpy())
        for name, g, r in zip(("details", "approximation", "reconstruction"), got, (d_ref, a_ref, y_ref)):
            err = float(np.max(np.abs(g - r)))
            print(f"  row {b} {name}: max|diff| = {err:.3e}")
            if f64 and not (flags & nat.FLAG_FMA):
                assert np.array_equal(g, r), f"{name} row {b} not bit-exact ({err:.3e})"
            else:
                assert err <= tol, f"{name} row {b}: {err:.3e} > {tol:.3e}"


def same_bits(a, b):
    import torch
    for name, u, v in zip(("details", "approximation", "reconstruction"), a, b):
        assert torch.equal(u, v), f"{name}: VW_LEVEL_CT=1 differs from VW_LEVEL_CT=0"


@pytest.mark.parametrize("fma", [False, True], ids=["exact", "fma"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-N{s[1]}-J{s[2]}")
@pytest.mark.parametrize("w", WAVELETS, ids=lambda w: w.name())
def test_periodic_forward_inverse(engine, w, shape, fma):
    import torch
    dt, n, J = shape
    B = 5
    flags = nat.FLAG_FMA if fma else 0
    x = torch.empty((B, n), dtype=torch.float64 if dt == "f64" else torch.float32, device="cuda")
    engine.fill_uniform(x, 101)
    for pol in POLICIES:
        on = fwd_inv(engine, x, w, O.PERIODIC, J, flags, VW_LEVEL_CT=1, **pol)
        off = fwd_inv(engine, x, w, O.PERIODIC, J, flags, VW_LEVEL_CT=0, **pol)
        same_bits(on, off)
        check_rows(x, on, w, J, flags, (0, B // 2, B - 1))
        check_rows(x, off, w, J, flags, (0, B // 2, B - 1))


@pytest.mark.parametrize("fma", [False, True], ids=["exact", "fma"])
def test_persistent_workgroup_walks_to_a_second_row(engine, fma):
    """A batch larger than the persistent forward's grid (resident workgroups per CU x CUs): some workgroups
    take a second row through the full-slab path, its LDS-DMA prefetch included.  A 64-thread workgroup is one
    wave and a CU holds at most 32 waves, so 32 per CU bounds the resident count from above whatever the LDS
    and register limits allow; + 3 rows.  At this batch the inverse is the one-buffer k_inverse_seq."""
    import torch
    w, n, J = Daubechies.DB4, 512, 6
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 32 * cus + 3
    flags = nat.FLAG_FMA if fma else 0
    x = torch.empty((B, n), dtype=torch.float64, device="cuda")
    engine.fill_uniform(x, 103)
    on = fwd_inv(engine, x, w, O.PERIODIC, J, flags, VW_LEVEL_CT=1)
    off = fwd_inv(engine, x, w, O.PERIODIC, J, flags, VW_LEVEL_CT=0)
    same_bits(on, off)
    check_rows(x, on, w, J, flags, (0, B // 2, B - 1))
    check_rows(x, off, w, J, flags, (0, B // 2, B - 1))


def signals(B, n, seed):
    return np.stack([O.java_random_signal(n, seed + b) for b in range(B)])


@pytest.mark.parametrize("boundary", [O.SYMMETRIC, O.ZERO_PADDING], ids=["S", "Z"])
def test_other_boundaries_keep_their_paths(engine, boundary):
    """SYMMETRIC (alignment shifts: offsets that are no multiple of the vector width) and ZERO_PADDING
    (pairwise sums) through reconstruct: bit-exact under both settings."""
    w, n, J = Daubechies.DB4, 512, 4
    x = signals(5, n, 41)
    tx = vw.MultiLevelMODWTTransform(w, vw.BoundaryMode(boundary))
    for ct in (1, 0):
        for pol in POLICIES:
            with engine.options(VW_LEVEL_CT=ct, **pol):
                res = tx.decompose(x, J)
                y = tx.reconstruct(res)
            for b in (0, 2, 4):
                d_ref, a_ref = O.decompose(x[b], *lohi(w), boundary, J)
                assert np.array_equal(res.details_array[:, b, :], d_ref), f"details row {b} ct={ct}"
                assert np.array_equal(res.approximation_array[b], a_ref), f"approximation row {b} ct={ct}"
                y_ref = O.reconstruct(d_ref, a_ref, *rlohi(w), boundary, w.wavelet_id)
                assert np.array_equal(y[b], y_ref), f"reconstruction row {b} ct={ct}"


def test_swt_denoise_thresholds(engine):
    """SWT denoise: the thresholds are applied on the inverse's detail loads (the thr path of k_inverse_seq
    under VW_INV_BUF=1, of k_inverse_db under the small-batch default)."""
    w, n, J = Daubechies.DB4, 512, 4
    x = signals(5, n, 43)
    swt = vw.VectorWaveSwtAdapter(w, vw.BoundaryMode.PERIODIC)
    ref = [O.swt_denoise(x[b], *lohi(w), O.PERIODIC, J, wavelet_id=w.wavelet_id) for b in range(5)]
    for ct in (1, 0):
        for pol in POLICIES:
            with engine.options(VW_LEVEL_CT=ct, **pol):
                y, thr = swt.denoise(x, J, return_thresholds=True)
            for b in range(5):
                assert thr[b] == ref[b][1], f"threshold row {b} ct={ct}"
                assert np.array_equal(y[b], ref[b][0]), f"denoised row {b} ct={ct}"


def test_ragged_rows_take_the_checked_path(engine):
    """N = 500: 250 vectors over 63 threads x 4 leave the last slab ragged, so neither the persistent forward
    nor the full-slab inverse may run; the strided levels still use the compile-time bodies."""
    w, n, J = Daubechies.DB4, 500, 3
    x = signals(5, n, 47)
    outs = []
    for ct in (1, 0):
        for pol in POLICIES:
            with engine.options(VW_LEVEL_CT=ct, **pol):
                det, app = engine.forward(x, *lohi(w), w.wavelet_id, O.PERIODIC, J, 0)
                y = engine.inverse(det, app, *rlohi(w), w.wavelet_id, O.PERIODIC, J, 0)
            for b in (0, 2, 4):
                d_ref, a_ref = O.decompose(x[b], *lohi(w), O.PERIODIC, J, core=False)
                assert np.array_equal(det[:, b, :], d_ref), f"details row {b} ct={ct}"
                assert np.array_equal(app[b], a_ref), f"approximation row {b} ct={ct}"
                assert np.array_equal(y[b], O.reconstruct(d_ref, a_ref, *rlohi(w), O.PERIODIC, w.wavelet_id))
            with engine.options(VW_LEVEL_CT=ct, **pol):
                outs.append(engine.forward(x, *lohi(w), w.wavelet_id, O.PERIODIC, J, nat.FLAG_FMA))
    for d_, a_ in outs[1:]:
        assert np.array_equal(d_, outs[0][0]) and np.array_equal(a_, outs[0][1])
