"""fp32 parity: the float kernels against a bit-level reference.

The reference has no fp32 path, but the engine's fp32 arithmetic is fully specified: the kernels compile with
fp-contract off, EXACT is ``acc + x * f`` with one rounding each (the packed forward form included), and the taps
are ``float(h * (1 / sqrt 2))`` rounded once.  tests/restatement_generic.py is that arithmetic in numpy.float32
(bit-equal to the C restatement at float64: tests/test_restatement_generic_cpu.py), so:

  EXACT fp32 == the float32 restatement bit for bit, and within 1e-5 * max|x| * J of the fp64 restatement;
  FMA fp32 == the float32 restatement with ``fma=True`` bit for bit (``fmaf(x, f, acc)`` per tap, the ZERO_PADDING
  inverse ``acc + fmaf(lo, a, round(hi * d))``: the correctly rounded primitive, tests/test_restatement_fma_cpu.py),
  within that bar as well, and bit-equal across kernel policies.

fp32 vectors hold 4 elements (fp64: 2): the shapes cover every N mod 4, row tails of 1..3 elements, halos rounded to
4, SYMMETRIC shifts that are no multiple of 4, leading dimensions that break the row alignment, and host memory.
Inputs are uniform in [-1, 1) rounded to float32; no product goes subnormal.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import Coiflet, Daubechies, Haar, Symlet, Wavelet

import restatement_generic as G

pytestmark = pytest.mark.gpu

SYN28 = Wavelet("syn28", G.synthetic_filter(28)[0])
SYN9 = Wavelet("syn9", G.synthetic_filter(9)[0])
FILTERS = [Haar.INSTANCE, Daubechies.DB4, Symlet.SYM8, Coiflet.COIF5, SYN28]
ALL = {w.name(): w for w in FILTERS + [SYN9]}
BOUNDARIES = [O.PERIODIC, O.SYMMETRIC, O.ZERO_PADDING]
BIDS = ["P", "S", "Z"]
F32 = np.float32


def lohi(w):
    return w.lowPassDecomposition(), w.highPassDecomposition()


@functools.lru_cache(maxsize=None)
def inputs(B, n, seed=5):
    x = O.fill_uniform(B * n, seed).reshape(B, n).astype(F32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name, boundary, B, n, J, mask=None, approx_zero=False):
    """float32 restatement (d, a, y), fp64 restatement (d, a, y) and float32 FMA restatement (d, a, y, y of the EXACT
    planes) of the same float32 input, computed once."""
    w = ALL[name]
    x = inputs(B, n)
    m = (1 << J) - 1 if mask is None else mask
    d32, a32 = G.decompose(x, *lohi(w), boundary, J, dtype=F32)
    y32 = G.reconstruct(d32, a32, *lohi(w), boundary, w.wavelet_id, detail_mask=m, approx_zero=approx_zero, dtype=F32)
    d64, a64, y64 = np.empty((J, B, n)), np.empty((B, n)), np.empty((B, n))
    for b in range(B):
        d64[:, b, :], a64[b] = O.decompose(x[b].astype(np.float64), *lohi(w), boundary, J, core=boundary != O.PERIODIC)
        y64[b] = O.reconstruct(d64[:, b, :], a64[b], *lohi(w), boundary, w.wavelet_id, detail_mask=m,
                               approx_zero=approx_zero)
    df, af = G.decompose(x, *lohi(w), boundary, J, dtype=F32, fma=True)
    kw = dict(detail_mask=m, approx_zero=approx_zero, dtype=F32, fma=True)
    yf = G.reconstruct(df, af, *lohi(w), boundary, w.wavelet_id, **kw)
    yf32 = G.reconstruct(d32, a32, *lohi(w), boundary, w.wavelet_id, **kw)   # the FMA inverse of the EXACT planes
    out = (d32, a32, y32, d64, a64, y64, (df, af, yf, yf32))
    for a in out[:6] + out[6]:
        a.setflags(write=False)
    return out


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def exact(a, b):
    a, b = host(a), host(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    if not np.array_equal(a, b):
        diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
        i = np.unravel_index(np.argmax(diff), a.shape)
        raise AssertionError(f"not bit-exact: {int(np.count_nonzero(a != b))} of {a.size} differ, "
                             f"max |diff| = {diff.max():.3e} at {i}")


def within(a, b, tol):
    err = float(np.max(np.abs(host(a).astype(np.float64) - b)))
    assert err <= tol, (err, tol)


def tol_of(x, J):
    return 1e-5 * float(np.max(np.abs(x))) * J


def run(engine, w, x, boundary, J, flags, d_in=None, a_in=None, mask=0xFFFFFFFF, approx_zero=False):
    det, app = engine.forward(x, *lohi(w), w.wavelet_id, boundary, J, flags)
    d_in = det if d_in is None else d_in
    a_in = app if a_in is None else a_in
    y = engine.inverse(d_in, None if approx_zero else a_in, *lohi(w), w.wavelet_id, boundary, J, flags,
                       detail_mask=mask, approx_zero=approx_zero, shape=tuple(x.shape))
    if isinstance(x, torch.Tensor):
        torch.cuda.synchronize()
    return det, app, y


def check_policies(engine, w, boundary, B, n, J, policies):
    d32, a32, y32, d64, a64, y64, (df, af, yf, _) = reference(w.name(), boundary, B, n, J)
    x = torch.from_numpy(np.array(inputs(B, n))).cuda()
    tol = tol_of(inputs(B, n), J)
    for flags in (0, nat.FLAG_FMA):
        outs = []
        for opts in policies:
            with engine.options(**opts):
                outs.append(run(engine, w, x, boundary, J, flags))
        for opts, out in zip(policies[1:], outs[1:]):
            for t0, t1 in zip(outs[0], out):
                assert torch.equal(t0, t1), (opts, "fma" if flags else "exact")
        det, app, y = outs[0]
        assert det.dtype == torch.float32 and y.dtype == torch.float32
        if not flags:
            exact(det, d32)
            exact(app, a32)
            exact(y, y32)
        else:
            exact(det, df)
            exact(app, af)
            exact(y, yf)
        within(det, d64, tol)
        within(app, a64, tol)
        within(y, y64, tol)


# ---- 1. fused path ------------------------------------------------------------------------------------------
POLICIES = [dict(), dict(VW_INV_BUF=1), dict(VW_INV_BUF=2), dict(VW_BLK=0)]


@pytest.mark.parametrize("w", FILTERS, ids=lambda w: w.name())
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
@pytest.mark.parametrize("n", [66, 67, 1024, 1025, 1026, 1027])   # every N mod 4; 1024: the persistent forward's smallest
def test_fused_path(engine, w, boundary, n):
    J = min(4, O.max_levels(n, w.filter_length))
    assert J >= 1
    check_policies(engine, w, boundary, 3, n, J, POLICIES)


# ---- 2. per-level path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [Daubechies.DB4, Symlet.SYM8], ids=lambda w: w.name())
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
@pytest.mark.parametrize("n", [4000, 4001, 4002, 4003])
def test_per_level_path(engine, w, boundary, n):
    J = 5 if boundary == O.PERIODIC else 4
    check_policies(engine, w, boundary, 3, n, J, [dict(VW_FORCE_TILED=1, VW_MULTI_TILE=256)])


# ---- 3. masks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [SYN28, SYN9], ids=lambda w: w.name())
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
@pytest.mark.parametrize("tiled,n", [(0, 514), (1, 2002)], ids=["fused", "tiled"])   # N = 2 mod 4: a half-filled last vector
def test_partial_reconstruction(engine, w, boundary, tiled, n):
    B, J = 3, 3
    tol = tol_of(inputs(B, n), J)
    for mask in (0b110, 0b001):
        for az in (False, True):
            d32, a32, y32, d64, a64, y64, (_, _, _, yf32) = reference(w.name(), boundary, B, n, J, mask, az)
            d, a = torch.from_numpy(np.array(d32)).cuda(), torch.from_numpy(np.array(a32)).cuda()
            with engine.options(VW_FORCE_TILED=tiled):
                ys = [engine.inverse(d, None if az else a, *lohi(w), w.wavelet_id, boundary, J, flags, detail_mask=mask,
                                     approx_zero=az, shape=(B, n)) for flags in (0, nat.FLAG_FMA)]
            torch.cuda.synchronize()
            exact(ys[0], y32)
            exact(ys[1], yf32)
            for y in ys:
                within(y, y64, tol)


# ---- 4. leading dimension ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("pad", [1, 2, 4])   # fp32: 1, 2 break the row alignment; fp64: 1 does
def test_forward_leading_dimension(engine, dt, pad):
    """vw_modwt_forward_* on rows of a wider buffer (ldx > N) against the restatement.  Every kernel the call can
    reach takes the row alignment from the host (vec_io / io_aligned / deep's lda test in vw_plan.cpp all include
    ldx % V == 0), so ldx % V != 0 runs the scalar row loads."""
    w, B, N, J = Daubechies.DB4, 5, 1024, 4
    tdt = torch.float32 if dt == "f32" else torch.float64
    big = torch.empty((B, N + pad), dtype=tdt, device="cuda")
    engine.fill_uniform(big, 9)
    xh = big[:, :N].cpu().numpy()
    lib = nat.load()
    fn = lib.vw_modwt_forward_f32 if dt == "f32" else lib.vw_modwt_forward_f64
    tol = tol_of(xh, J) if dt == "f32" else 1e-12
    d64, a64 = np.empty((J, B, N)), np.empty((B, N))
    for b in range(B):
        d64[:, b, :], a64[b] = O.decompose(xh[b].astype(np.float64), *lohi(w), O.PERIODIC, J, core=False)
    for flags in (0, nat.FLAG_FMA):
        det = torch.empty((J, B, N), dtype=tdt, device="cuda")
        app = torch.empty((B, N), dtype=tdt, device="cuda")
        st = fn(engine.ctx, ctypes.c_void_p(big.data_ptr()), B, N, N + pad, nat.taps_array(lohi(w)[0]),
                nat.taps_array(lohi(w)[1]), w.filter_length, w.wavelet_id, O.PERIODIC, J, flags,
                ctypes.c_void_p(det.data_ptr()), ctypes.c_void_p(app.data_ptr()))
        assert st == 0, nat.last_error()
        torch.cuda.synchronize()
        if not flags:
            if dt == "f32":
                d32, a32 = G.decompose(xh, *lohi(w), O.PERIODIC, J, dtype=F32)
                exact(det, d32)
                exact(app, a32)
            else:
                exact(det, d64)
                exact(app, a64)
        else:
            df, af = G.decompose(xh, *lohi(w), O.PERIODIC, J, dtype=F32 if dt == "f32" else np.float64, fma=True)
            exact(det, df)
            exact(app, af)
        within(det, d64, tol)
        within(app, a64, tol)


# ---- 5. host memory ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
@pytest.mark.parametrize("n", [1024, 1027])
def test_host_memory(engine, boundary, n):
    """numpy float32 in and out: the staged host path of the fp32 entry points."""
    w, B, J = Symlet.SYM8, 3, 4
    d32, a32, y32, d64, a64, y64, (df, af, yf, _) = reference(w.name(), boundary, B, n, J)
    x = np.array(inputs(B, n))
    det, app, y = run(engine, w, x, boundary, J, 0)
    assert isinstance(det, np.ndarray) and det.dtype == F32 and y.dtype == F32
    exact(det, d32)
    exact(app, a32)
    exact(y, y32)
    det, app, y = run(engine, w, x, boundary, J, nat.FLAG_FMA)
    exact(det, df)
    exact(app, af)
    exact(y, yf)
    tol = tol_of(x, J)
    within(det, d64, tol)
    within(app, a64, tol)
    within(y, y64, tol)


# ---- 6. VW_FLAG_VALIDATE -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_validate_reports_the_index(engine, device):
    w = Daubechies.DB4
    x = np.array(inputs(3, 256))
    x[1, 77] = np.nan
    xin = torch.from_numpy(x).cuda() if device else x
    with pytest.raises(vw.InvalidSignalException) as ei:
        engine.forward(xin, *lohi(w), w.wavelet_id, O.PERIODIC, 3, nat.FLAG_VALIDATE)
    assert ei.value.index == 77
