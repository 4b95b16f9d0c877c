"""Every form of a launcher that picks its kernel at run time, one after another on one engine in one process.

A kernel's dynamic-LDS limit is raised past the 64 KiB default once per kernel instantiation and device
(vw_launch_k.h launch_k owns that flag, one per kernel).  A launcher that paired a kernel with a sibling's flag would
leave the kernel at the default and fail its first large launch with an error status -- only in a process where the
sibling ran first.  So the forms that share a launcher run back to back here, in one process, at shapes whose plans
need more than 64 KiB wherever the form can need it, and every result is compared with the restatement as
tests/test_gpu_inverse_waves.py does: EXACT bit for bit, FMA within 1e-12.

The forms, with the plans the planner prints for them (fp64, B = 3; db4 = 8 taps, db8 = 16 taps, J = 4):
  forward, launch_forward_fused / _persist / _blk
    fused, no history    N = 8192, VW_FWD_PERSIST=0          k_forward_fused<NV = 8, HIST = 0>   66,000 B
    fused, history       N = 8192, BatchStreamingMODWT ZERO  k_forward_fused<NV = 8, HIST = 1>   66,000 B
    persistent           N = 4096 (NV = 4, 512 threads)      k_forward_persist                   66,464 B
    register-blocked     N = 8192, db8                       k_forward_blk<NV = 8>               75,120 B
  inverse, launch_inverse_fused (run_inverse_fused_nv's seven forms)
    pair                 N = 8192, one level, ZERO_PADDING   k_inverse_fused<NV = 8>            131,232 B
    two-buffer           N = 8192, VW_INV_BUF=2              k_inverse_db<NV = 8>               132,000 B
    one-buffer           N = 8192, SYMMETRIC, VW_INV_BUF=1   k_inverse_seq<NV = 8>               66,016 B
    register-blocked     N = 8192, db8                       k_inverse_blk<NV = 8>               75,056 B
    full-slab, not PLAIN N = 4096, SWT denoise, VW_INV_BUF=1 k_inverse_seq<NV = 4, FULL>         33,232 B
    PLAIN, 6 / 8 waves   N = 4096, VW_INV_BUF=1              k_inverse_seq<NV = 4, FULL, PLAIN>  33,232 B
  multi-level inverse, launch_inverse_multi (VW_FORCE_TILED=1, N = 8192)
    NI = 8               VW_MULTI_INV_TILE=3968              k_inverse_multi<NI = 8>             67,776 B
    NI = 4               default tile                        k_inverse_multi<NI = 4>             43,136 B
The full-slab forms exist at NV = 4 only, whose workgroups have at most 512 threads: N <= 4096 in fp64, one level
buffer, 33 KiB -- they cannot need the raised limit, and N = 4096 is their largest shape.  NI = 4 keeps
(tile + reach) / V <= 1536 vectors and at most 1024 at level 1: its two padded regions stay below 64,064 B, and with
a larger tile the planner falls back to NI = 8 -- so NI = 4 runs at its default plan.
"""
import numpy as np
import pytest

from oracle import oracle as O
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import Daubechies

pytestmark = pytest.mark.gpu

B, J = 3, 4
DB4, DB8 = Daubechies.DB4, Daubechies.DB8


def lohi(w):
    return w.lowPassDecomposition(), w.highPassDecomposition()


def rlohi(w):
    return w.lowPassReconstruction(), w.highPassReconstruction()


def signals(n, seed):
    return np.stack([O.java_random_signal(n, seed + b) for b in range(B)])


def compare(got, ref, flags, what):
    got = np.asarray(got.cpu().numpy() if hasattr(got, "cpu") else got)
    err = float(np.max(np.abs(got - ref)))
    print(f"  {what} flags={flags}: max|got - ref| = {err:.3e}")
    if flags & nat.FLAG_FMA:
        assert err <= 1e-12, f"{what}: {err:.3e} > 1e-12"
    else:
        assert np.array_equal(got, ref), f"{what} not bit-exact ({err:.3e})"


_REF = {}


def reference(w, n, boundary, seed):
    """x [B][n] and, per row, the restatement's (details, approx, y); computed once per case."""
    key = (w.name(), n, boundary, seed)
    if key not in _REF:
        x = signals(n, seed)
        rows = []
        for b in range(B):
            d, a = O.decompose(x[b], *lohi(w), boundary, J, core=boundary != O.PERIODIC)
            rows.append((d, a, O.reconstruct(d, a, *rlohi(w), boundary, w.wavelet_id)))
        _REF[key] = (x, rows)
    return _REF[key]


def forward(engine, w, n, boundary, seed, flags, **opts):
    import torch
    x, rows = reference(w, n, boundary, seed)
    with engine.options(**opts):
        det, app = engine.forward(torch.from_numpy(x).cuda(), *lohi(w), w.wavelet_id, boundary, J, flags)
        torch.cuda.synchronize()
    for b in range(B):
        compare(det[:, b, :], rows[b][0], flags, f"{opts} details row {b}")
        compare(app[b], rows[b][1], flags, f"{opts} approx row {b}")


def inverse(engine, w, n, boundary, seed, flags, **opts):
    """The inverse from the restatement's own coefficients (EXACT: the device's, bit for bit)."""
    import torch
    _, rows = reference(w, n, boundary, seed)
    det = torch.from_numpy(np.stack([r[0] for r in rows], axis=1)).cuda()
    app = torch.from_numpy(np.stack([r[1] for r in rows])).cuda()
    with engine.options(**opts):
        y = engine.inverse(det, app, *rlohi(w), w.wavelet_id, boundary, J, flags)
        torch.cuda.synchronize()
    for b in range(B):
        compare(y[b], rows[b][2], flags, f"{opts} y row {b}")


def test_forward_forms_one_after_another(engine):
    for flags in (0, nat.FLAG_FMA):
        forward(engine, DB4, 8192, O.PERIODIC, 301, flags, VW_FWD_PERSIST=0)  # fused, no history
        forward(engine, DB4, 4096, O.PERIODIC, 302, flags)                    # persistent
        forward(engine, DB8, 8192, O.PERIODIC, 303, flags)                    # register-blocked
    # fused with streaming history: two blocks, the second reads the history the first wrote (EXACT facade)
    n = 8192
    x = signals(2 * n, 304)
    st = vw.BatchStreamingMODWT(DB4, vw.BoundaryMode(O.ZERO_PADDING), J)
    refs = [O.StreamRestatement(*lohi(DB4), O.ZERO_PADDING, J) for _ in range(B)]
    for k in range(2):
        out = st.processMultiLevel(x[:, k * n:(k + 1) * n])
        for b in range(B):
            d_ref, a_ref = refs[b].process(x[b, k * n:(k + 1) * n])
            compare(out.detailPerLevel[:, b, :], d_ref, 0, f"stream block {k} details row {b}")
            compare(out.finalApprox[b], a_ref, 0, f"stream block {k} approx row {b}")
    st.close()
    forward(engine, DB4, 8192, O.PERIODIC, 301, 0, VW_FWD_PERSIST=0)  # and the sibling again, after the history form


def test_inverse_forms_one_after_another(engine):
    import torch
    for flags in (0, nat.FLAG_FMA):
        # pair form: one level, ZERO_PADDING (MODWTTransform.inverse)
        x = signals(8192, 311)
        ad = [O.modwt_forward(x[b], *lohi(DB4), O.ZERO_PADDING) for b in range(B)]
        a = torch.from_numpy(np.stack([r[0] for r in ad])).cuda()
        d = torch.from_numpy(np.stack([r[1] for r in ad])).cuda()
        y = engine.inverse1(a, d, *rlohi(DB4), O.ZERO_PADDING, flags)
        torch.cuda.synchronize()
        for b in range(B):
            compare(y[b], O.modwt_inverse(*ad[b], *rlohi(DB4), O.ZERO_PADDING), flags, f"pair y row {b}")
        inverse(engine, DB4, 8192, O.PERIODIC, 312, flags, VW_INV_BUF=2)    # two-buffer
        inverse(engine, DB4, 8192, O.SYMMETRIC, 313, flags, VW_INV_BUF=1)   # general one-buffer
        inverse(engine, DB8, 8192, O.PERIODIC, 314, flags)                  # register-blocked
        inverse(engine, DB4, 4096, O.PERIODIC, 315, flags, VW_INV_BUF=1, VW_INV_WAVES=6)  # PLAIN, 6 waves
        inverse(engine, DB4, 4096, O.PERIODIC, 315, flags, VW_INV_BUF=1, VW_INV_WAVES=8)  # PLAIN, 8 waves
    # full-slab, not PLAIN: the thresholded SWT denoise (EXACT facade)
    x = signals(4096, 316)
    swt = vw.VectorWaveSwtAdapter(DB4, vw.BoundaryMode.PERIODIC)
    with engine.options(VW_INV_BUF=1):
        y, thr = swt.denoise(x, J, return_thresholds=True)
    for b in range(B):
        y_ref, t_ref = O.swt_denoise(x[b], *lohi(DB4), O.PERIODIC, J, wavelet_id=DB4.wavelet_id)
        assert thr[b] == t_ref, f"threshold row {b}"
        compare(y[b], y_ref, 0, f"denoised row {b}")
    inverse(engine, DB4, 8192, O.SYMMETRIC, 313, 0, VW_INV_BUF=1)  # the one-buffer sibling again, after its full-slab forms


def test_multilevel_inverse_forms_one_after_another(engine):
    for flags in (0, nat.FLAG_FMA):
        inverse(engine, DB4, 8192, O.PERIODIC, 321, flags, VW_FORCE_TILED=1, VW_MULTI_NI=4)
        inverse(engine, DB4, 8192, O.PERIODIC, 321, flags, VW_FORCE_TILED=1, VW_MULTI_NI=8, VW_MULTI_INV_TILE=3968)
