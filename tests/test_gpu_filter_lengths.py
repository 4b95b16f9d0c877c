"""Filter-length sweep: every tap count the dispatcher treats differently, on every kernel family.

The unrolled tap list instantiates 2..30-tap kernels; the rest of the suite runs 2, 4, 6, 8, 12, 16, 18 and 30 only.
Here: the listed-but-untested lengths (sym5 10, sym7 14, db10 20, coif4 24) and lengths outside the list, which
run the runtime-L kernels -- even 22, 28, 32, 60, 64 (the ABI's limit) and odd 3, 9, 31, as synthetic banks
(tests/restatement_generic.synthetic_filter: pseudo-random taps with sum|lo| = sqrt(2), QMF high-pass, VW_WID_OTHER).

Bars (the suite's own): EXACT bit-exact against the CPU restatement; FMA bit-exact against the restatement's FMA
form (tests/restatement_generic.py ``fma=True``: ``fma(x, f, acc)`` per tap, the ZERO_PADDING inverse
``acc + fma(lo, a, round(hi * d))``), within 1e-12 of the EXACT one (|x| <= 1 and a gain of at
most 1 per level: at most L * 2^-53 * max|x| per level, below 3e-14 over the J <= 5 levels here) and bit-equal
between kernel policies.  PERIODIC references use the batch semantics (core=False: no FFT region); calls go to the
engine without validation flags, on device tensors, so the persistent / register-blocked choices are reachable.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd.errors import VW_ERR_ARG
from vectorwave_amd.wavelets import WID_OTHER, Coiflet, Daubechies, Symlet, Wavelet

import restatement_bi as RB
import restatement_generic as G

pytestmark = pytest.mark.gpu

LISTED = [Symlet.SYM5, Symlet.SYM7, Daubechies.DB10, Coiflet.COIF4]          # 10, 14, 20, 24 taps
UNLISTED = [Wavelet(f"syn{L}", G.synthetic_filter(L)[0]) for L in (22, 28, 32, 60, 64, 3, 9, 31)]
FILTERS = LISTED + UNLISTED
BY_LEN = {w.filter_length: w for w in FILTERS}
BOUNDARIES = [O.PERIODIC, O.SYMMETRIC, O.ZERO_PADDING]
BIDS = ["P", "S", "Z"]
FMA_TOL = 1e-12


def test_filter_catalogue():
    assert sorted(BY_LEN) == [3, 9, 10, 14, 20, 22, 24, 28, 31, 32, 60, 64]
    for w in UNLISTED:
        assert w.wavelet_id == WID_OTHER
        lo, hi = G.synthetic_filter(w.filter_length)
        assert w.lowPassDecomposition() == lo and w.highPassDecomposition() == hi   # Wavelet's QMF is the issue's
        assert abs(sum(abs(v) for v in lo) - np.sqrt(2.0)) < 1e-15


def lohi(w):
    return w.lowPassDecomposition(), w.highPassDecomposition()


@functools.lru_cache(maxsize=None)
def signals(B, n, seed=7):
    x = np.stack([O.java_random_signal(n, seed + b) for b in range(B)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name, boundary, B, n, J, mask=None, approx_zero=False):
    """(details [J,B,N], approx [B,N], y [B,N]) of the restatement; computed once per case and shared."""
    w = next(f for f in FILTERS if f.name() == name)
    x = signals(B, n)
    det, app, y = np.empty((J, B, n)), np.empty((B, n)), np.empty((B, n))
    full = (1 << J) - 1
    for b in range(B):
        det[:, b, :], app[b] = O.decompose(x[b], *lohi(w), boundary, J, core=boundary != O.PERIODIC)
        y[b] = O.reconstruct(det[:, b, :], app[b], *lohi(w), boundary, w.wavelet_id,
                             detail_mask=full if mask is None else mask, approx_zero=approx_zero)
    for a in (det, app, y):
        a.setflags(write=False)
    return det, app, y


@functools.lru_cache(maxsize=None)
def reference_fma(name, boundary, B, n, J, mask=None, approx_zero=False):
    """The FMA restatement: (details, approx) of the signals, y of those planes, and y of the EXACT reference's planes
    (what the tests that feed the inverse the reference's coefficients get); computed once per case and shared."""
    w = next(f for f in FILTERS if f.name() == name)
    d_ref, a_ref, _ = reference(name, boundary, B, n, J, mask, approx_zero)
    kw = dict(detail_mask=(1 << J) - 1 if mask is None else mask, approx_zero=approx_zero, fma=True)
    det, app = G.decompose(signals(B, n), *lohi(w), boundary, J, fma=True)
    y_own = G.reconstruct(det, app, *lohi(w), boundary, w.wavelet_id, **kw)
    y_of_ref = G.reconstruct(d_ref, a_ref, *lohi(w), boundary, w.wavelet_id, **kw)
    for a in (det, app, y_own, y_of_ref):
        a.setflags(write=False)
    return det, app, y_own, y_of_ref


def exact(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.shape == b.shape
    if not np.array_equal(a, b):
        i = np.unravel_index(np.argmax(np.abs(a - b)), a.shape)
        raise AssertionError(f"not bit-exact: max |diff| = {np.max(np.abs(a - b)):.3e} at {i}")


def close(a, b):
    err = float(np.max(np.abs(a.cpu().numpy() - np.asarray(b))))
    assert err <= FMA_TOL, err


def round_trip(engine, w, x, boundary, J, flags, mask=0xFFFFFFFF, approx_zero=False, det_app=None):
    """forward, then inverse of (det_app or the forward's own outputs), on the device."""
    det, app = engine.forward(x, *lohi(w), w.wavelet_id, boundary, J, flags)
    d_in, a_in = det_app if det_app is not None else (det, app)
    y = engine.inverse(d_in, a_in, *lohi(w), w.wavelet_id, boundary, J, flags, detail_mask=mask,
                       approx_zero=approx_zero)
    torch.cuda.synchronize()
    return det, app, y


def check_both_modes(engine, w, boundary, B, n, J):
    """EXACT bit-exact (forward, inverse of the forward's outputs == inverse of the reference's); FMA bit-exact
    against the FMA restatement (forward; inverse of the EXACT reference's planes) and within 1e-12."""
    d_ref, a_ref, y_ref = reference(w.name(), boundary, B, n, J)
    x = torch.from_numpy(np.array(signals(B, n))).cuda()
    det, app, y = round_trip(engine, w, x, boundary, J, 0)
    exact(det, d_ref)
    exact(app, a_ref)
    exact(y, y_ref)
    det, app, y = round_trip(engine, w, x, boundary, J, nat.FLAG_FMA,
                             det_app=(torch.from_numpy(np.array(d_ref)).cuda(), torch.from_numpy(np.array(a_ref)).cuda()))
    d_fma, a_fma, _, y_fma = reference_fma(w.name(), boundary, B, n, J)
    exact(det, d_fma)
    exact(app, a_fma)
    exact(y, y_fma)
    close(det, d_ref)
    close(app, a_ref)
    close(y, y_ref)


# ---- 1. fused path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", FILTERS, ids=lambda w: w.name())
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
@pytest.mark.parametrize("n", [512, 509])   # 509: scalar I/O, ragged last slab
def test_fused_path(engine, w, boundary, n):
    check_both_modes(engine, w, boundary, 5, n, 3)   # J = 3 keeps L_J <= N for L = 64


# ---- 2. kernel policies, PERIODIC -----------------------------------------------------------------------------
POLICIES = [dict(), dict(VW_BLK=0), dict(VW_INV_BUF=1), dict(VW_INV_BUF=2), dict(VW_NV=8)]


@pytest.mark.parametrize("w", FILTERS, ids=lambda w: w.name())
@pytest.mark.parametrize("B,n", [(5, 512), (3, 4096)], ids=["512", "4096"])   # 4096: the persistent forward's shape
def test_kernel_policies_periodic(engine, w, B, n):
    J = 3
    d_ref, a_ref, y_ref = reference(w.name(), O.PERIODIC, B, n, J)
    x = torch.from_numpy(np.array(signals(B, n))).cuda()
    for flags in (0, nat.FLAG_FMA):
        outs = []
        for opts in POLICIES:
            with engine.options(**opts):
                outs.append(round_trip(engine, w, x, O.PERIODIC, J, flags))
        for opts, out in zip(POLICIES[1:], outs[1:]):
            for t0, t1 in zip(outs[0], out):
                assert torch.equal(t0, t1), (opts, "fma" if flags else "exact")
        det, app, y = outs[0]
        if flags:
            d_fma, a_fma, y_fma, _ = reference_fma(w.name(), O.PERIODIC, B, n, J)
            exact(det, d_fma)
            exact(app, a_fma)
            exact(y, y_fma)
            close(det, d_ref)
            close(app, a_ref)
        else:
            exact(det, d_ref)
            exact(app, a_ref)
            exact(y, y_ref)


# ---- 3. NV = 8 register-blocked forward ------------------------------------------------------------------------
@pytest.mark.parametrize("L", [10, 14, 20, 24, 28])
def test_nv8_blocked_forward(engine, L):
    w, B, n, J = BY_LEN[L], 3, 8192, 3   # 8192: the smallest N that plans NV = 8 in fp64
    d_ref, a_ref, y_ref = reference(w.name(), O.PERIODIC, B, n, J)
    x = torch.from_numpy(np.array(signals(B, n))).cuda()
    for flags in (0, nat.FLAG_FMA):
        outs = []
        for fwd8 in (0, 1):
            with engine.options(VW_BLK_FWD8=fwd8):
                outs.append(round_trip(engine, w, x, O.PERIODIC, J, flags))
        for t0, t1 in zip(*outs):
            assert torch.equal(t0, t1), "fma" if flags else "exact"
        det, app, y = outs[1]
        if flags:
            d_fma, a_fma, y_fma, _ = reference_fma(w.name(), O.PERIODIC, B, n, J)
            exact(det, d_fma)
            exact(app, a_fma)
            exact(y, y_fma)
            close(det, d_ref)
            close(app, a_ref)
        else:
            exact(det, d_ref)
            exact(app, a_ref)
            exact(y, y_ref)


# ---- 4. per-level path (the only place the runtime-L tile and multi-level kernels run) ------------------------------
def halo_exceeds_lds(L, J):
    """The per-level path's documented refusal (VW_ERR_UNSUPPORTED, "halo exceeds LDS"): the level's halo leaves
    less than a 64-vector tile of the 160 KiB of LDS (fp64: vectors of 2)."""
    V, lds_elems = 2, 160 * 1024 // 8
    hp = -(-(L - 1) * (1 << (J - 1)) // V) * V
    return (lds_elems - hp - 2 * V) // V * V < 64 * V


@pytest.mark.parametrize("w", FILTERS, ids=lambda w: w.name())
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
@pytest.mark.parametrize("tile", [128, -1], ids=["tile128", "tile-default"])
def test_per_level_path(engine, w, boundary, tile):
    J = 5 if boundary == O.PERIODIC else 4
    with engine.options(VW_FORCE_TILED=1, VW_MULTI_TILE=tile):
        for n in (2000, 2001):
            if halo_exceeds_lds(w.filter_length, J):   # asserted, not skipped (no length here reaches it)
                x = torch.from_numpy(np.array(signals(2, n))).cuda()
                with pytest.raises(NotImplementedError, match="exceeds LDS"):
                    engine.forward(x, *lohi(w), w.wavelet_id, boundary, J, 0)
                continue
            check_both_modes(engine, w, boundary, 2, n, J)


# ---- 5. partial reconstruction -----------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [28, 9])
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
@pytest.mark.parametrize("tiled", [0, 1], ids=["fused", "tiled"])
def test_partial_reconstruction(engine, L, boundary, tiled):
    w, B, J = BY_LEN[L], 3, 3
    n = 2000 if tiled else 512
    for mask in (0b110, 0b001):
        for az in (False, True):
            d_ref, a_ref, y_ref = reference(w.name(), boundary, B, n, J, mask, az)
            d, a = torch.from_numpy(np.array(d_ref)).cuda(), torch.from_numpy(np.array(a_ref)).cuda()
            with engine.options(VW_FORCE_TILED=tiled):
                y = engine.inverse(d, None if az else a, *lohi(w), w.wavelet_id, boundary, J, 0, detail_mask=mask,
                                   approx_zero=az, shape=(B, n))
                yf = engine.inverse(d, None if az else a, *lohi(w), w.wavelet_id, boundary, J, nat.FLAG_FMA,
                                    detail_mask=mask, approx_zero=az, shape=(B, n))
            torch.cuda.synchronize()
            exact(y, y_ref)
            exact(yf, reference_fma(w.name(), boundary, B, n, J, mask, az)[3])
            close(yf, y_ref)


# ---- 6. streaming history kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [28, 9])
@pytest.mark.parametrize("boundary", [O.ZERO_PADDING, O.SYMMETRIC], ids=["Z", "S"])
def test_streaming_history(engine, L, boundary):
    w, blk, J = BY_LEN[L], 256, 2
    x = signals(2, blk * 3, 17)
    st = vw.BatchStreamingMODWT(w, vw.BoundaryMode(boundary), J)
    refs = [O.StreamRestatement(*lohi(w), boundary, J) for _ in range(2)]
    for k in range(3):
        out = st.processMultiLevel(x[:, k * blk:(k + 1) * blk])
        for b in range(2):
            d_ref, a_ref = refs[b].process(x[b, k * blk:(k + 1) * blk])
            exact(out.detailPerLevel[:, b, :], d_ref)
            exact(out.finalApprox[b], a_ref)
    assert st.getMinFlushTailLength() == L - 1
    tail = st.flushMultiLevel(L - 1)
    for b in range(2):
        d_ref, a_ref = refs[b].flush(L - 1)
        exact(tail.detailPerLevel[:, b, :], d_ref)
        exact(tail.finalApprox[b], a_ref)
    st.close()


# ---- 7. single level (vw_modwt1_*) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [28, 9])
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
@pytest.mark.parametrize("n", [7, 64, 1000])   # 7 < L
def test_single_level(engine, L, boundary, n):
    w = BY_LEN[L]
    x = np.array(signals(4, n, 11))
    tx = vw.MODWTTransform(w, vw.BoundaryMode(boundary))
    r = tx.forwardBatch(x)
    for b in range(4):
        a_ref, d_ref = O.modwt_forward(x[b], *lohi(w), boundary)
        exact(r[b].approximationCoeffs(), a_ref)
        exact(r[b].detailCoeffs(), d_ref)
        exact(tx.inverse(r[b]), O.modwt_inverse(a_ref, d_ref, *lohi(w), boundary))
    ys = tx.inverseBatch(r)
    for b in range(4):
        a_ref, d_ref = O.modwt_forward(x[b], *lohi(w), boundary)
        exact(ys[b], O.modwt_inverse(a_ref, d_ref, *lohi(w), boundary, batch_optimized=n >= 64))
    # FMA: fma(x, f, acc) per forward tap, the pairwise inverse acc + fma(lo, a, round(hi * d)) in every boundary
    txf = vw.MODWTTransform(w, vw.BoundaryMode(boundary), fma=True)
    rf = txf.forwardBatch(x)
    a_fma, d_fma = RB.forward1(x, *lohi(w), boundary, fma=True)
    ysf = txf.inverseBatch(rf)
    for b in range(4):
        exact(rf[b].approximationCoeffs(), a_fma[b])
        exact(rf[b].detailCoeffs(), d_fma[b])
        exact(txf.inverse(rf[b]), RB.inverse1(a_fma[b], d_fma[b], *lohi(w), boundary, fma=True))
        exact(ysf[b], RB.inverse1(a_fma[b], d_fma[b], *lohi(w), boundary, batch_sym=n >= 64, fma=True))


# ---- 8. SWT denoise ----------------------------------------------------------------------------------------------------
def test_swt_denoise_28_taps(engine):
    w, n, J = BY_LEN[28], 1024, 3
    x = np.array(signals(3, n, 29))
    y, thr = vw.VectorWaveSwtAdapter(w, vw.BoundaryMode.PERIODIC).denoise(x, J, return_thresholds=True)
    xd = torch.from_numpy(x).cuda()   # device tensors: the unvalidated kernels' choices too
    yd, thrd = engine.denoise(xd, *lohi(w), w.wavelet_id, O.PERIODIC, J, -1.0, True, 0, want_thresholds=True)
    torch.cuda.synchronize()
    for b in range(3):
        y_ref, t_ref = O.swt_denoise(x[b], *lohi(w), O.PERIODIC, J, wavelet_id=w.wavelet_id)
        assert thr[b] == t_ref and float(thrd[b]) == t_ref
        exact(y[b], y_ref)
        exact(yd[b], y_ref)


# ---- 9. argument edges ------------------------------------------------------------------------------------------------
def test_filter_length_limits(engine):
    # L = 64 is the longest the ABI accepts (bit-exact: test_fused_path[...-syn64]); 65 and 0 are argument errors
    n, B, J = 512, 2, 1
    x = torch.from_numpy(np.array(signals(B, n))).cuda()
    det = torch.empty((J, B, n), dtype=torch.float64, device="cuda")
    app = torch.empty((B, n), dtype=torch.float64, device="cuda")
    w = BY_LEN[64]
    d, a = engine.forward(x, *lohi(w), WID_OTHER, O.PERIODIC, J, 0)
    d_ref, a_ref, _ = reference(w.name(), O.PERIODIC, B, n, J)
    exact(d, d_ref)
    exact(a, a_ref)
    taps = nat.taps_array(G.synthetic_filter(64)[0] + [0.0])
    lib = nat.load()
    for L in (65, 0):
        st = lib.vw_modwt_forward_f64(engine.ctx, ctypes.c_void_p(x.data_ptr()), B, n, n, taps, taps, L, WID_OTHER,
                                      O.PERIODIC, J, 0, ctypes.c_void_p(det.data_ptr()), ctypes.c_void_p(app.data_ptr()))
        assert st == VW_ERR_ARG, (L, st)
        st = lib.vw_modwt_inverse_f64(engine.ctx, ctypes.c_void_p(det.data_ptr()), ctypes.c_void_p(app.data_ptr()), B, n,
                                      taps, taps, L, WID_OTHER, O.PERIODIC, J, 1, 0, 0, ctypes.c_void_p(x.data_ptr()))
        assert st == VW_ERR_ARG, (L, st)
