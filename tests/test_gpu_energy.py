"""Wavelet energy per level on the GPU (vw_modwt_energy_f64 / vw_energy_planes_f64) against the sequential
restatement (tests/energy_restatement.py: np.add.accumulate(c*c)[-1] over oracle.decompose's planes).

Exact mode is compared bit for bit.  VW_FLAG_TREE_SUMS only reorders the N non-negative terms of a sum whose
coefficients are identical to exact mode's: any summation order has relative error <= (N-1)u, u = 2^-53, so
two orders differ by less than 2(N-1)u: the bar is |E_tree - E_seq| <= N * 2^-52 * E_seq.  With VW_FLAG_FMA the
coefficients move by at most the project's own bar of 1e-12 (tests/test_gpu_headline.py), so
|sum (c+e)^2 - sum c^2| <= 2e-12 * sqrt(N * E) + N * 1e-24, plus the reordering term.
"""
import functools
from ctypes import c_void_p

import numpy as np
import pytest

import energy_restatement as ER
import restatement_generic as G
from oracle import oracle as O
from vectorwave_amd import _native as nat
from vectorwave_amd import errors
from vectorwave_amd.wavelets import Coiflet, Daubechies, Haar, Symlet

pytestmark = pytest.mark.gpu

PAD = 3                      # ldx = N + 3: unaligned rows
NS = [7, 64, 129, 1001, 1024, 4096]
BS = [1, 3, 70]
BOUNDS = {"P": O.PERIODIC, "S": O.SYMMETRIC, "Z": O.ZERO_PADDING}
CORE = nat.FLAG_CORE_LEVELS | nat.FLAG_FFT_SWITCH


def _filter(name):
    """(lo, hi, wavelet_id)"""
    if name == "syn9":
        lo, hi = G.synthetic_filter(9)
        return lo, hi, 0
    w = {"haar": Haar.INSTANCE, "db4": Daubechies.DB4, "sym8": Symlet.SYM8, "coif5": Coiflet.COIF5}[name]
    return list(w.lowPassDecomposition()), list(w.highPassDecomposition()), w.wavelet_id


FILTERS = ["haar", "db4", "sym8", "coif5", "syn9"]


@functools.lru_cache(maxsize=None)
def _signals(N):
    """[70, N + PAD]: random rows of mixed scale, row 1 all zeros, NaN in the padding columns."""
    rng = np.random.default_rng(1000 + N)
    x = rng.standard_normal((max(BS), N + PAD)) * np.exp(rng.uniform(-3, 3, (max(BS), 1)))
    x[1] = 0.0
    x[:, N:] = np.nan
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(fname, bname, N, J):
    lo, hi, _ = _filter(fname)
    e = ER.energies(_signals(N)[:, :N], lo, hi, BOUNDS[bname], J, core=_core(bname, N))
    e.setflags(write=False)
    return e


def _core(bname, N):
    """oracle.decompose's mode.  PERIODIC at N >= 1024: MultiLevelMODWTTransform.decompose sends the levels with
    N/8 < L_j <= N/2 through a real FFT, which the engine's forward replaces by the direct sum (the same sum for
    a power-of-two N, not the FFT's roundings; include/vectorwave_amd.h VW_FLAG_FFT_SWITCH).  The energies are
    exact with respect to the forward's coefficients, so the oracle's direct loops (core=False: no FFT, no cap)
    are the restatement there."""
    return not (bname == "P" and N >= 1024)


def _levels(fname, N):
    """J = 1 and the largest J the forward accepts (none when the filter does not fit N)."""
    L = len(_filter(fname)[0])
    mx = O.max_levels(N, L)
    return [] if mx < 1 else sorted({1, mx})


def _to(kind, a):
    if kind == "host":
        return np.array(a)
    import torch
    return torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _tree_bound(ref, N):
    return N * 2.0 ** -52 * ref


# ---- 1. exact mode ------------------------------------------------------------------------------
@pytest.mark.parametrize("bname", list(BOUNDS))
@pytest.mark.parametrize("fname", FILTERS)
def test_exact_bit_equal(engine, fname, bname):
    lo, hi, wid = _filter(fname)
    ran = 0
    for N in NS:
        for J in _levels(fname, N):
            ref = _reference(fname, bname, N, J)
            for B in BS:
                for kind in ("device", "host"):
                    x = _to(kind, _signals(N)[:B])
                    for fused in (0, -1):   # forced off / the default policy
                        with engine.options(VW_ENERGY_FUSED=fused):
                            got = _host(engine.energy(x, lo, hi, wid, BOUNDS[bname], J, CORE, N=N))
                        assert got.shape == (J + 1, B)
                        assert _same_bits(got, ref[:, :B]), (fname, bname, N, J, B, kind, fused)
                        ran += 1
            # the all-zero row: +0.0 in every plane
            if J:
                assert not np.signbit(ref[:, 1]).any() and (ref[:, 1] == 0.0).all()
    assert ran > 0


# ---- 2. vw_energy_planes_f64 ----------------------------------------------------------------------
@pytest.mark.parametrize("bname", list(BOUNDS))
def test_planes_of_the_forwards_own_output(engine, bname):
    lo, hi, wid = _filter("db4")
    for N in (64, 1001, 4096):
        J = O.max_levels(N, len(lo))
        x = _to("device", np.ascontiguousarray(_signals(N)[:, :N]))
        det, app = engine.forward(x, lo, hi, wid, BOUNDS[bname], J, CORE)
        got = _host(engine.energy_planes(det, app))
        assert _same_bits(got, _reference("db4", bname, N, J)), (bname, N)
        got_h = engine.energy_planes(_host(det), _host(app))
        assert _same_bits(got_h, got)


@pytest.mark.parametrize("N", [7, 31, 32, 33, 1001])       # below one tile, at it, not a multiple of it
@pytest.mark.parametrize("J,B", [(0, 1), (2, 21), (1, 32), (4, 13), (7, 25)])   # (J+1)*B = 1, 63, 64, 65, 200
def test_planes_chain_edges(engine, J, B, N):
    rng = np.random.default_rng(J * 100 + B + N)
    app = rng.standard_normal((B, N))
    det = rng.standard_normal((J, B, N))
    ref = ER.planes_energies(det, app)
    for kind in ("device", "host"):
        got = _host(engine.energy_planes(_to(kind, det) if J else None, _to(kind, app)))
        assert _same_bits(got, ref), (kind, J, B, N)
        tree = _host(engine.energy_planes(_to(kind, det) if J else None, _to(kind, app), nat.FLAG_TREE_SUMS))
        assert (np.abs(tree - ref) <= _tree_bound(ref, N)).all()


# ---- 3. tree mode ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bname", list(BOUNDS))
@pytest.mark.parametrize("fname", FILTERS)
def test_tree_sums_within_the_reordering_bound(engine, fname, bname):
    lo, hi, wid = _filter(fname)
    worst = 0.0
    for N in NS:
        for J in _levels(fname, N):
            ref = _reference(fname, bname, N, J)
            # padded rows (ldx = N + 3: the runtime-L kernel), packed rows (aligned: the tap-unrolled kernels)
            for kind, packed in (("device", False), ("device", True), ("host", False)):
                x = _to(kind, np.ascontiguousarray(_signals(N)[:, :N]) if packed else _signals(N))
                for fused in (-1, 0):   # the fused kernel where it applies / forward, then tree sums of the planes
                    with engine.options(VW_ENERGY_FUSED=fused):
                        got = _host(engine.energy(x, lo, hi, wid, BOUNDS[bname], J, nat.FLAG_CORE_LEVELS |
                                                  nat.FLAG_TREE_SUMS, N=N))
                        again = _host(engine.energy(x, lo, hi, wid, BOUNDS[bname], J, nat.FLAG_CORE_LEVELS |
                                                    nat.FLAG_TREE_SUMS, N=N))
                    assert _same_bits(got, again), "tree sums must be deterministic"
                    err, bar = np.abs(got - ref), _tree_bound(ref, N)
                    worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
                    assert (err <= bar).all(), (fname, bname, N, J, kind, packed, fused, float((err / np.maximum(bar, 1e-300)).max()))
                    assert (got[:, 1] == 0.0).all() and not np.signbit(got[:, 1]).any()
    print(f"{fname} {bname}: largest |E_tree - E_seq| / (N 2^-52 E_seq) = {worst:.4f}")


# ---- 4. tree mode with FMA ------------------------------------------------------------------------
@pytest.mark.parametrize("fname", ["db4", "sym8", "syn9"])
def test_tree_sums_fma(engine, fname):
    import torch
    lo, hi, wid = _filter(fname)
    for N, B in ((1001, 5), (4096, 9)):
        J = O.max_levels(N, len(lo))
        x = torch.empty((B, N), dtype=torch.float64, device="cuda")
        engine.fill_uniform(x, 77 + N)
        ref = ER.energies(x.cpu().numpy(), lo, hi, O.PERIODIC, J, core=_core("P", N))
        bar = 2e-12 * np.sqrt(N * ref) + N * 2.0 ** -52 * ref + N * 1e-24
        for fused in (-1, 0):
            with engine.options(VW_ENERGY_FUSED=fused):
                got = _host(engine.energy(x, lo, hi, wid, O.PERIODIC, J,
                                          nat.FLAG_CORE_LEVELS | nat.FLAG_TREE_SUMS | nat.FLAG_FMA))
            assert (np.abs(got - ref) <= bar).all(), (fname, N, fused, float((np.abs(got - ref) / bar).max()))


# ---- 5. fused-path limits ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,fused", [(16384, True), (16386, False)])
def test_fused_path_limits(engine, N, fused):
    lo, hi, wid = _filter("db4")
    J, B = 6, 2
    xh = np.random.default_rng(N).standard_normal((B, N))
    ref = ER.energies(xh, lo, hi, O.PERIODIC, J, core=False)
    x = _to("device", xh)
    engine.energy(x, lo, hi, wid, O.PERIODIC, J, nat.FLAG_TREE_SUMS)   # (workspace growth is not what is timed)
    engine.synchronize()
    engine.enable_timing(True)
    engine.reset_timing()
    try:
        got = _host(engine.energy(x, lo, hi, wid, O.PERIODIC, J, nat.FLAG_TREE_SUMS))
        engine.synchronize()
        n_fused = engine.kernel_time("energy_fused")[1]
        n_tree = engine.kernel_time("energy_tree")[1]
        n_fwd = engine.kernel_time("forward")[1] + engine.kernel_time("forward_level")[1]
    finally:
        engine.enable_timing(False)
        engine.reset_timing()
    assert (n_fused, n_tree, n_fwd > 0) == ((1, 0, False) if fused else (0, 1, True))
    assert (np.abs(got - ref) <= _tree_bound(ref, N)).all()


# ---- 6. more rows than the grid ---------------------------------------------------------------------
def test_more_rows_than_the_grid(engine):
    lo, hi, wid = _filter("db4")
    N, B, J = 64, 5000, 3
    rng = np.random.default_rng(5000)
    xh = rng.standard_normal((B, N)) * np.exp(rng.uniform(-2, 2, (B, 1)))
    ref = ER.energies(xh, lo, hi, O.PERIODIC, J)
    got = _host(engine.energy(_to("device", xh), lo, hi, wid, O.PERIODIC, J, nat.FLAG_TREE_SUMS))
    bad = np.argwhere(~(np.abs(got - ref) <= _tree_bound(ref, N)))
    assert bad.size == 0, bad[:8]


# ---- 7. status parity with the forward ----------------------------------------------------------------
def _status_pair(engine, xh, lo, hi, wid, boundary, J, flags, B=None, N=None):
    """(status, error index) of vw_modwt_forward_f64 and of vw_modwt_energy_f64 on host arrays."""
    B = xh.shape[0] if B is None else B
    N = xh.shape[1] if N is None else N
    lib, ctx = engine.lib, engine.ctx
    tl, th = nat.taps_array(lo), nat.taps_array(hi)
    det, app = np.empty((max(J, 1), max(B, 1), max(N, 1))), np.empty((max(B, 1), max(N, 1)))
    out = np.empty((max(J, 0) + 1, max(B, 1)))
    P = lambda a: c_void_p(a.ctypes.data)  # noqa: E731
    fl = flags | nat.FLAG_HOST_MEMORY
    s1 = lib.vw_modwt_forward_f64(ctx, P(xh), B, N, xh.shape[1], tl, th, len(lo), wid, boundary, J, fl, P(det), P(app))
    i1 = nat.last_error_index()
    s2 = lib.vw_modwt_energy_f64(ctx, P(xh), B, N, xh.shape[1], tl, th, len(lo), wid, boundary, J, fl, P(out))
    i2 = nat.last_error_index()
    return (s1, i1), (s2, i2)


def test_status_parity_with_the_forward(engine):
    lo, hi, wid = _filter("db4")
    L = len(lo)
    J = 3
    LJ = (L - 1) * (1 << (J - 1)) + 1
    for N, want in ((LJ - 1, errors.VW_ERR_LEVEL), (LJ, 0)):   # just below and at L_J under CORE_LEVELS
        xh = np.random.default_rng(N).standard_normal((2, N))
        for tree in (0, nat.FLAG_TREE_SUMS):
            f, e = _status_pair(engine, xh, lo, hi, wid, O.PERIODIC, J, nat.FLAG_CORE_LEVELS | tree)
            assert f == e and f[0] == want, (N, f, e)
    xh = np.random.default_rng(1).standard_normal((2, 256))
    for Jbad in (0, 10, 25):                                    # J = 0, above the core cap, above the engine limit
        for flags in (nat.FLAG_CORE_LEVELS, 0):
            f, e = _status_pair(engine, xh, lo, hi, wid, O.PERIODIC, Jbad, flags)
            assert f == e, (Jbad, flags, f, e)
            if Jbad in (0, 25) or flags:
                assert f[0] == errors.VW_ERR_LEVEL
    f, e = _status_pair(engine, xh, lo, hi, wid, O.PERIODIC, 2, 0, B=0)          # empty batch
    assert f == e and f[0] == errors.VW_ERR_EMPTY
    f, e = _status_pair(engine, xh, lo, hi, wid, 7, 2, 0)                          # unsupported boundary
    assert f == e and f[0] == errors.VW_ERR_BOUNDARY
    bad = xh.copy()
    bad[1, 37] = np.nan
    for tree in (0, nat.FLAG_TREE_SUMS):
        f, e = _status_pair(engine, bad, lo, hi, wid, O.PERIODIC, 2, nat.FLAG_CORE_LEVELS | nat.FLAG_VALIDATE | tree)
        assert f == e and f == (errors.VW_ERR_NONFINITE, 37), (f, e)


@pytest.mark.parametrize("tree", [False, True])
def test_ref_nonfinite_energies_follow_the_forwards_planes(engine, tree):
    lo, hi, wid = _filter("db4")
    xh = np.random.default_rng(3).standard_normal((4, 512))
    xh[2, 100] = np.inf
    xh[3, 7] = np.nan
    x = _to("device", xh)
    det, app = engine.forward(x, lo, hi, wid, O.PERIODIC, 4, nat.FLAG_REF_NONFINITE)
    ref = ER.planes_energies(_host(det), _host(app))
    got = _host(engine.energy(x, lo, hi, wid, O.PERIODIC, 4,
                              nat.FLAG_REF_NONFINITE | (nat.FLAG_TREE_SUMS if tree else 0)))
    if tree:
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref))
        assert (np.abs(got[fin] - ref[fin]) <= _tree_bound(ref[fin], 512)).all()
    else:
        assert np.array_equal(got, ref, equal_nan=True)
    assert np.isfinite(got[:, :2]).all() and not np.isfinite(got[:, 2:]).all()


# ---- 8. graph capture ---------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, nat.FLAG_TREE_SUMS], ids=["exact", "tree"])
def test_graph_capture_replays_the_energy_call(engine, flags):
    import torch
    lo, hi, wid = _filter("db4")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.empty((16, 1024), dtype=torch.float64, device="cuda")
        engine.fill_uniform(x, 9)
        eager = engine.energy(x, lo, hi, wid, O.PERIODIC, 5, flags).clone()   # (also grows the workspace)
        torch.cuda.synchronize()
        g = engine.capture(lambda: engine.energy(x, lo, hi, wid, O.PERIODIC, 5, flags))
        g.result.fill_(float("nan"))
        g.launch(1)
        g.launch(1)
        torch.cuda.synchronize()
        assert torch.equal(g.result, eager)
        g.close()
    if not flags:
        assert _same_bits(eager.cpu().numpy(), ER.energies(x.cpu().numpy(), lo, hi, O.PERIODIC, 5, core=False))
