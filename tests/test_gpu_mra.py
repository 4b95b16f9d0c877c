"""Multiresolution analysis on the GPU (vw_mra_planes_* / vw_modwt_mra_*, the facades over them).

Component c of coefficient planes is DEFINED as the masked inverse (detail_mask = c ? 1 << (c-1) : 0,
approx_zero = c != 0).  References: oracle.reconstruct with those masks at fp64 (the C restatement runs every
upsampled tap, O(N * L_J) per level, so it is applied to the first and the last row of a batch; every row is also
compared with tests/restatement_generic.reconstruct at float64, which tests/test_restatement_generic_cpu.py proves
equal to the oracle bit for bit), restatement_generic at float32 for fp32.  EXACT results are compared bit for
bit, signs of zeros included.

Tolerances of the FMA runs are the existing inverse tests': fp64 max-abs < 1e-12 on unit-scale planes
(tests/test_gpu_headline.py), fp32 1e-5 * max|planes| * J against the fp64 restatement
(tests/test_gpu_f32_parity.py tol_of).  Beside them the FMA runs are compared bit for bit with the FMA restatement
of the path that ran: k_mra's branch passes (mra_restatement.mra, ``fma=True``) or the loop path's masked inverses
(mra_restatement.mra_by_masks, ``fma=True``) -- the same bytes for PERIODIC and SYMMETRIC, two different fixed
sequences for ZERO_PADDING, whose masked pairwise term rounds the single product before adding it.
"""
import functools
from ctypes import c_void_p

import numpy as np
import pytest

import mra_restatement as M
import restatement_generic as G
from oracle import oracle as O
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import WID_OTHER, Coiflet, Daubechies, Haar, Symlet, get_wavelet

pytestmark = pytest.mark.gpu

BOUNDS = {"P": O.PERIODIC, "S": O.SYMMETRIC, "Z": O.ZERO_PADDING}
FILTERS = ["haar", "db4", "sym8", "coif5", "syn9", "syn22"]
NS = [64, 61, 256, 1024, 4096]
BS = [1, 5]
DTYPES = {"f64": np.float64, "f32": np.float32}
MAXB = max(BS)


def _filter(name):
    """(lo, hi, wavelet_id): the reconstruction pair (== the decomposition pair: orthogonal or synthetic)."""
    if name.startswith("syn"):
        lo, hi = G.synthetic_filter(int(name[3:]))
        return lo, hi, WID_OTHER
    w = {"haar": Haar.INSTANCE, "db4": Daubechies.DB4, "sym8": Symlet.SYM8, "coif5": Coiflet.COIF5}[name]
    return list(w.lowPassReconstruction()), list(w.highPassReconstruction()), w.wavelet_id


def _fits(L, J, N):
    return (L - 1) * (1 << (J - 1)) + 1 <= N


def _largest(L, N):
    """The largest J the planes call accepts with L_J <= N (the engine's limit is 24 levels)."""
    J = 0
    while J < 24 and _fits(L, J + 1, N):
        J += 1
    return J


def _grid(fname):
    """[(N, J, runs)] of one filter: J in {1, 3, largest allowed}; only L_J > N is skipped."""
    L = len(_filter(fname)[0])
    out = []
    for N in NS:
        for J in sorted({1, 3, max(_largest(L, N), 1)}):
            out.append((N, J, _fits(L, J, N)))
    return out


@functools.lru_cache(maxsize=None)
def _planes(N, J):
    """(details [J, 5, N], approx [5, N]) at unit scale: generic rows, row 1 all zeros, row 2 coarsely quantised,
    row 3 a single spike per plane (mostly exact zeros)."""
    rng = np.random.default_rng(77 * N + J)
    det = rng.uniform(-1.0, 1.0, (J, MAXB, N))
    app = rng.uniform(-1.0, 1.0, (MAXB, N))
    det[:, 1] = 0.0
    app[1] = 0.0
    det[:, 2] = np.round(det[:, 2] * 8.0) / 8.0
    app[2] = np.round(app[2] * 8.0) / 8.0
    spike = np.zeros(N)
    spike[N // 3] = -1.0
    det[:, 3] = spike
    app[3] = spike
    det.setflags(write=False)
    app.setflags(write=False)
    return det, app


def _masks(c):
    return ((1 << (c - 1)) if c else 0), c != 0


@functools.lru_cache(maxsize=None)
def _reference(fname, bname, N, J, dname):
    """[J+1, 5, N] in the element type: restatement_generic's masked reconstructions of the planes rounded to it."""
    lo, hi, wid = _filter(fname)
    dt = DTYPES[dname]
    det, app = _planes(N, J)
    ref = np.stack([G.reconstruct(det.astype(dt), app.astype(dt), lo, hi, BOUNDS[bname], wid, *_masks(c), dtype=dt)
                    for c in range(J + 1)])
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _reference_fma(fname, bname, N, J, dname):
    """(k_mra's sequence, the loop path's sequence), each [J+1, 5, N] in the element type, FMA mode."""
    lo, hi, wid = _filter(fname)
    dt = DTYPES[dname]
    det, app = _planes(N, J)
    out = (M.mra(det.astype(dt), app.astype(dt), lo, hi, BOUNDS[bname], wid, dtype=dt, fma=True),
           M.mra_by_masks(det.astype(dt), app.astype(dt), lo, hi, BOUNDS[bname], wid, dtype=dt, fma=True))
    for a in out:
        a.setflags(write=False)
    return out


def _oracle_rows(fname, bname, N, J, rows):
    """{row: [J+1, N]} from the C restatement (fp64)."""
    lo, hi, wid = _filter(fname)
    det, app = _planes(N, J)
    return {b: np.stack([O.reconstruct(det[:, b, :], app[b], lo, hi, BOUNDS[bname], wid, detail_mask=_masks(c)[0],
                                       approx_zero=_masks(c)[1]) for c in range(J + 1)]) for b in rows}


def _dev(a, dname):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64 if dname == "f64" else torch.float32, device="cuda")


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _run_planes(engine, fname, bname, N, J, B, dname, flags=0):
    lo, hi, wid = _filter(fname)
    det, app = _planes(N, J)
    return _host(engine.mra_planes(_dev(det[:, :B], dname), _dev(app[:B], dname), lo, hi, wid, BOUNDS[bname], flags))


# ---- 1. EXACT components ---------------------------------------------------------------------------
def test_grid_coverage():
    """At least 90 % of the stated grid runs (a skip cannot hide a failure); pure arithmetic on the grid."""
    cells = [runs for f in FILTERS for (_, _, runs) in _grid(f)]
    assert sum(cells) >= 0.9 * len(cells), (sum(cells), len(cells))


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("bname", list(BOUNDS))
@pytest.mark.parametrize("fname", FILTERS)
def test_exact_components_bit_equal(engine, fname, bname, dname):
    ran = 0
    for N, J, runs in _grid(fname):
        if not runs:
            continue
        ref = _reference(fname, bname, N, J, dname)
        for B in BS:
            got = _run_planes(engine, fname, bname, N, J, B, dname)
            assert got.shape == (J + 1, B, N)
            assert _same_bits(got, ref[:, :B]), (fname, bname, N, J, B, dname)
            ran += 1
        # k_mra also where the default policy prefers the loop (listed lengths past its unrolled bodies)
        with engine.options(VW_MRA_FUSED=2):
            assert _same_bits(_run_planes(engine, fname, bname, N, J, MAXB, dname), ref), (fname, bname, N, J, dname)
        if dname == "f64":   # the C restatement itself, on the first and the last row
            for b, want in _oracle_rows(fname, bname, N, J, (0, MAXB - 1)).items():
                assert _same_bits(ref[:, b], want), ("restatement vs oracle", fname, bname, N, J, b)
    assert ran == 2 * sum(runs for (_, _, runs) in _grid(fname)) and ran > 0


# ---- 2. FMA ------------------------------------------------------------------------------------------
def _fused_ran(engine, fn):
    """(fn's result, whether k_mra ran): the timing families count the launches, as test_paths_are_the_planned_ones."""
    engine.reset_timing()
    engine.enable_timing(True)
    try:
        out = fn()
        engine.synchronize()
        mra_n, inv_n = engine.kernel_time("mra")[1], engine.kernel_time("inverse")[1] + engine.kernel_time("inverse_level")[1]
    finally:
        engine.enable_timing(False)
        engine.reset_timing()
    assert (mra_n > 0) != (inv_n > 0), (mra_n, inv_n)
    return out, mra_n > 0


def _check_fma_bits(engine, default_out, fname, bname, N, J, dname):
    """The default call, k_mra forced (VW_MRA_FUSED=2) and the loop path (VW_MRA_FUSED=0), each against the FMA
    restatement of the path that ran."""
    fused_ref, loop_ref = _reference_fma(fname, bname, N, J, dname)
    if bname != "Z":
        assert _same_bits(fused_ref, loop_ref), ("the two FMA sequences", fname, bname, N, J, dname)
    paths = []
    for mode in (-1, 2, 0):
        with engine.options(VW_MRA_FUSED=mode):
            got, fused = _fused_ran(engine, lambda: _run_planes(engine, fname, bname, N, J, MAXB, dname, nat.FLAG_FMA))
        assert _same_bits(got, fused_ref if fused else loop_ref), \
            (f"fma bits {fname} {bname} N={N} J={J} {dname} VW_MRA_FUSED={mode} k_mra ran={fused}: "
             f"{int(np.count_nonzero(got != fused_ref))} outputs differ from k_mra's sequence, "
             f"{int(np.count_nonzero(got != loop_ref))} from the loop path's")
        if mode == -1:
            assert _same_bits(got, default_out), ("timing changed the bits", fname, bname, N, J, dname)
        paths.append(fused)
    assert not paths[2], "VW_MRA_FUSED=0 ran k_mra"
    return paths


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("bname", list(BOUNDS))
@pytest.mark.parametrize("fname", FILTERS)
def test_fma_within_the_inverse_bars(engine, fname, bname, dname):
    """One N per body: 61 (runtime-L body, ragged rows) and 4096 (the tap-unrolled body where the length has one)."""
    L = len(_filter(fname)[0])
    ran = 0
    for N in (61, 4096):
        for J in sorted({1, 3, max(_largest(L, N), 1)}):
            if not _fits(L, J, N):
                continue
            raw = _run_planes(engine, fname, bname, N, J, MAXB, dname, nat.FLAG_FMA)
            _check_fma_bits(engine, raw, fname, bname, N, J, dname)
            got = raw.astype(np.float64)
            ref = np.asarray(_reference(fname, bname, N, J, "f64"))
            det, app = _planes(N, J)
            tol = 1e-12 if dname == "f64" else 1e-5 * max(np.max(np.abs(det)), np.max(np.abs(app))) * J
            err = float(np.max(np.abs(got - ref)))
            print(f"fma {fname} {bname} {dname} N={N} J={J}: max|err| = {err:.3e} (bar {tol:.3e})")
            assert err < tol, (fname, bname, N, J, dname, err, tol)
            ran += 1
    assert ran > 0


# ---- 3. more rows than resident workgroups -----------------------------------------------------------
def test_row_coverage(engine):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, N, J = 4 * cus + 3, 64, 2
    lo, hi, wid = _filter("db4")
    rng = np.random.default_rng(5)
    det, app = rng.uniform(-1, 1, (J, B, N)), rng.uniform(-1, 1, (B, N))
    got = _host(engine.mra_planes(_dev(det, "f64"), _dev(app, "f64"), lo, hi, wid, O.PERIODIC, 0))
    assert got.shape == (J + 1, B, N)
    for b in (0, B // 4, B // 2, (3 * B) // 4 + 1, B - 1):
        for c in range(J + 1):
            want = O.reconstruct(det[:, b, :], app[b], lo, hi, O.PERIODIC, wid, detail_mask=_masks(c)[0],
                                 approx_zero=_masks(c)[1])
            assert _same_bits(got[c, b], want), (b, c)


# ---- 4. the loop path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("bname", list(BOUNDS))
def test_loop_path_equals_default(engine, bname, dname):
    for fname, N, J in (("db4", 61, 3), ("db4", 1024, 6), ("sym8", 256, 4), ("syn9", 64, 3)):
        want = _run_planes(engine, fname, bname, N, J, MAXB, dname)
        with engine.options(VW_MRA_FUSED=0):
            got = _run_planes(engine, fname, bname, N, J, MAXB, dname)
        assert _same_bits(got, want), (fname, bname, N, J, dname)
        assert _same_bits(got, _reference(fname, bname, N, J, dname))


def test_paths_are_the_planned_ones(engine):
    """The default call on a row that fits runs k_mra once and no inverse; VW_MRA_FUSED=0, REF_NONFINITE and a row
    too long for two regions run J+1 inverses and no k_mra (timing families "mra" / "inverse" / "inverse_level")."""
    def counts(fn):
        engine.reset_timing()
        engine.enable_timing(True)
        try:
            fn()
            engine.synchronize()
            return engine.kernel_time("mra")[1], engine.kernel_time("inverse")[1] + engine.kernel_time("inverse_level")[1]
        finally:
            engine.enable_timing(False)
            engine.reset_timing()

    assert counts(lambda: _run_planes(engine, "db4", "P", 1024, 6, MAXB, "f64")) == (1, 0)
    assert counts(lambda: _run_planes(engine, "syn9", "S", 1024, 6, MAXB, "f32")) == (1, 0)
    # coif5 on aligned rows: the inverses have a 30-tap unrolled kernel, k_mra does not -- the loop (measured faster)
    assert counts(lambda: _run_planes(engine, "coif5", "S", 1024, 6, MAXB, "f32"))[0] == 0
    with engine.options(VW_MRA_FUSED=2):
        assert counts(lambda: _run_planes(engine, "coif5", "S", 1024, 6, MAXB, "f32")) == (1, 0)
    assert counts(lambda: _run_planes(engine, "db4", "P", 1024, 6, MAXB, "f64", nat.FLAG_REF_NONFINITE))[0] == 0
    with engine.options(VW_MRA_FUSED=0):
        m, inv = counts(lambda: _run_planes(engine, "db4", "P", 1024, 6, MAXB, "f64"))
    assert m == 0 and inv >= 7


# ---- 5. from signals -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("bname,N,J,flags", [("P", 1024, 6, nat.FLAG_CORE_LEVELS | nat.FLAG_FFT_SWITCH),
                                             ("P", 61, 3, 0), ("S", 256, 4, nat.FLAG_CORE_LEVELS), ("Z", 1024, 5, 0)],
                         ids=["P-fft-switch", "P-61", "S-256", "Z-1024"])
def test_signal_call_equals_forward_then_planes(engine, bname, N, J, flags, dname):
    w = Daubechies.DB4
    lo, hi, wid = list(w.lowPassDecomposition()), list(w.highPassDecomposition()), w.wavelet_id
    x = _dev(np.random.default_rng(N + J).uniform(-1, 1, (MAXB, N)), dname)
    det, app = engine.forward(x, lo, hi, wid, BOUNDS[bname], J, flags)
    want = _host(engine.mra_planes(det, app, lo, hi, wid, BOUNDS[bname], flags & ~nat.FLAG_FFT_SWITCH))
    got = _host(engine.mra(x, lo, hi, wid, BOUNDS[bname], J, flags))
    assert got.shape == (J + 1, MAXB, N) and _same_bits(got, want)
    if bname == "P":
        # the split is additive, and the PERIODIC inverse reconstructs: the components sum to x within the taps'
        # own precision (the round-trip bar of __graft_entry__.smoke, 1e-9; fp32: the f32 parity bar at |x| <= 1)
        tol = 1e-9 if dname == "f64" else 1e-5 * J
        assert float(np.max(np.abs(got.astype(np.float64).sum(axis=0) - _host(x).astype(np.float64)))) < tol


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_signal_call_error_statuses_are_the_forwards(engine, sfx):
    import torch
    w = Daubechies.DB4
    lo, hi = nat.taps_array(w.lowPassDecomposition()), nat.taps_array(w.highPassDecomposition())
    lib, ctx = engine.lib, engine.ctx
    dt = torch.float64 if sfx == "f64" else torch.float32
    B, N = 2, 64
    x = torch.zeros((B, N), dtype=dt, device="cuda")
    engine.bind_torch_stream()
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    mra, fwd = getattr(lib, f"vw_modwt_mra_{sfx}"), getattr(lib, f"vw_modwt_forward_{sfx}")
    cap = vw.max_levels(N, 8)
    refused = 0
    # J above the cap (with and without the FFT switch), far above it, and L_J = 225 > N without CORE_LEVELS
    for J, flags in ((cap + 1, nat.FLAG_CORE_LEVELS), (cap + 1, nat.FLAG_CORE_LEVELS | nat.FLAG_FFT_SWITCH),
                     (10, nat.FLAG_CORE_LEVELS), (25, 0), (6, 0)):
        out = torch.zeros((J + 1, B, N), dtype=dt, device="cuda")
        det = torch.zeros((J, B, N), dtype=dt, device="cuda")
        app = torch.zeros((B, N), dtype=dt, device="cuda")
        sf = fwd(ctx, P(x), B, N, N, lo, hi, 8, w.wavelet_id, 0, J, flags, P(det), P(app))
        mf = nat.last_error()
        sm = mra(ctx, P(x), B, N, N, lo, hi, 8, w.wavelet_id, 0, J, flags, P(out))
        assert sm == sf, (J, flags, sm, sf)
        if sf != 0:
            assert nat.last_error() == mf
            refused += 1
    torch.cuda.synchronize()
    assert refused >= 4


# ---- 6. a row that does not fit two LDS regions ---------------------------------------------------------
def test_long_row_runs_through_the_plan(engine):
    fname, bname, N, J, B = "sym8", "P", 16384, 8, 2
    lo, hi, wid = _filter(fname)
    rng = np.random.default_rng(9)
    det, app = rng.uniform(-1, 1, (J, B, N)), rng.uniform(-1, 1, (B, N))
    got = _host(engine.mra_planes(_dev(det, "f64"), _dev(app, "f64"), lo, hi, wid, BOUNDS[bname], 0))
    for c in range(J + 1):
        want = G.reconstruct(det, app, lo, hi, BOUNDS[bname], wid, *_masks(c))
        assert _same_bits(got[c], want), c
    for c in (0, J):   # the C restatement on the last row (every upsampled tap: the two ends of the cascade only)
        want = O.reconstruct(det[:, B - 1, :], app[B - 1], lo, hi, BOUNDS[bname], wid, detail_mask=_masks(c)[0],
                             approx_zero=_masks(c)[1])
        assert _same_bits(got[c, B - 1], want), c


# ---- 7. non-finite input ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bname", list(BOUNDS))
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
def test_nonfinite_rows_follow_the_masked_inverses(engine, bname, bad):
    fname, N, J = "db4", 256, 4
    lo, hi, wid = _filter(fname)
    det, app = (np.array(a) for a in _planes(N, J))
    det[1, 2, 17] = bad       # row 2, level 2
    app[4, N - 1] = bad       # row 4, the approximation
    d, a = _dev(det, "f64"), _dev(app, "f64")
    flags = nat.FLAG_REF_NONFINITE
    got = _host(engine.mra_planes(d, a, lo, hi, wid, BOUNDS[bname], flags))
    for c in range(J + 1):
        mask, az = _masks(c)
        want = _host(engine.inverse(d if mask else None, None if az else a, lo, hi, wid, BOUNDS[bname], J, flags,
                                    detail_mask=mask, approx_zero=az, shape=(MAXB, N)))
        assert _same_bits(got[c], want), (bname, c)
    assert not np.isfinite(got[:, 2]).all() and not np.isfinite(got[0, 4]).all()
    assert np.isfinite(got[:, 0]).all()


# ---- 8. graph capture ---------------------------------------------------------------------------------------
def test_captured_signal_call_replays_to_the_same_bits(engine):
    import torch
    w, B, N, J = Daubechies.DB4, 16, 1024, 5
    lo, hi = nat.taps_array(w.lowPassDecomposition()), nat.taps_array(w.highPassDecomposition())
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.empty((B, N), dtype=torch.float64, device="cuda")
        out = torch.empty((J + 1, B, N), dtype=torch.float64, device="cuda")
        engine.fill_uniform(x, 7)
        lib, ctx = engine.lib, engine.ctx
        P = lambda t: c_void_p(t.data_ptr())  # noqa: E731

        def step():
            assert lib.vw_modwt_mra_f64(ctx, P(x), B, N, N, lo, hi, len(lo), w.wavelet_id, 0, J, 0, P(out)) == 0

        step()   # the warm call: the workspace grows outside a capture only
        torch.cuda.synchronize()
        o0 = out.clone()
        g = engine.capture(step)
        out.fill_(float("nan"))
        g.launch(2)
        torch.cuda.synchronize()
        assert torch.equal(out, o0)
        g.close()
    # and the recorded result is the planes call's on the forward's coefficients
    det, app = engine.forward(x, list(w.lowPassDecomposition()), list(w.highPassDecomposition()), w.wavelet_id, 0, J, 0)
    want = engine.mra_planes(det, app, list(w.lowPassReconstruction()), list(w.highPassReconstruction()),
                             w.wavelet_id, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(o0, want)


# ---- 9. facades -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("bname", list(BOUNDS))
@pytest.mark.parametrize("wname", ["db4", "bior4.4"])
def test_facades_equal_stacked_extract_level(engine, wname, bname, kind):
    w = get_wavelet(wname)
    mode = vw.BoundaryMode(BOUNDS[bname])
    B, N, J = 3, 512, 3
    xh = np.random.default_rng(3).uniform(-1, 1, (B, N))
    x = xh if kind == "host" else _dev(xh, "f64")
    swt = vw.VectorWaveSwtAdapter(w, mode)
    tx = vw.MultiLevelMODWTTransform(w, mode)
    want = np.stack([_host(swt.extractLevel(x, J, c)) for c in range(J + 1)])
    for finite in (False, True):
        if finite and wname != "db4":
            continue
        assert _same_bits(_host(swt.extractAllLevels(x, J, finite=finite)), want), ("extractAllLevels", finite)
        assert _same_bits(_host(tx.mraBatch(x, J, finite=finite)), want), ("mraBatch", finite)
        assert _same_bits(_host(tx.mra(tx.decompose(x, J), finite=finite)), want), ("mra", finite)
    # one signal: [J+1, N]
    one = _host(swt.extractAllLevels(x[0], J))
    assert one.shape == (J + 1, N) and _same_bits(one, want[:, 0])
    # mraBatch validates as decompose does
    bad = xh.copy()
    bad[1, 5] = np.nan
    bad = bad if kind == "host" else _dev(bad, "f64")
    with pytest.raises(vw.errors.InvalidSignalException) as e1:
        tx.decompose(bad, J)
    with pytest.raises(vw.errors.InvalidSignalException) as e2:
        tx.mraBatch(bad, J)
    assert str(e1.value) == str(e2.value)
