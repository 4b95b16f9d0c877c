"""Where the kernels read and write: every case of tests/footprint_cases.py on guarded arenas (tests/guarded.py).

Every array of a call lives alone between two guard zones of at least max(N, 16384) + 64 elements that hold one NaN
bit pattern, as do the pad elements of padded rows and the payload of every output before the call.  Under each
shift pattern (no pointer, every pointer, each pointer alone one element off a 16-byte boundary) and for flags 0 and
VW_FLAG_FMA a case asserts:

  1. the status is VW_OK -- VW_FLAG_VALIDATE must not see the NaNs around the rows;
  2. guarded.check: no guard, shift slot, pad or input word changed, no output element was left unwritten;
  3. the payload equals the reference bit for bit: the restatement of the same operation, computed on the CPU from the
     payload values alone (oracle for fp64 EXACT, restatement_generic / restatement_bi / mra_restatement /
     energy_restatement / cwt_restatement / fin_restatement otherwise; the oracle's values for thresholds, sigma and
     median).  Forms without a bit-exact restatement (tree sums, the FMA forms of energy, CWT, analytics and denoise)
     must instead equal, bit for bit, the same call on plain, aligned, finite-padded tensors: neither alignment nor
     what lies around a row may reach a result.  No tolerance appears in this file;
  4. the case ran what it exists for, as far as the engine exposes it: launches per timing family (`forward` against
     `forward_level`, ...), `ref_nonfinite` for the fix-up, vw_graph_stats' fused pairs and vw_roundtrip_variant's
     keep.  Which kernel or step kinds a case selects under every pattern is pinned on the CPU
     (tests/test_plan_cpu.py).

In FMA mode the fix-up cases also show that poisoned pads recompute no row: a recomputed row would hold the
reference's EXACT bits, not the FMA restatement's."""
import functools
from ctypes import byref, c_void_p

import numpy as np
import pytest

from oracle import oracle as O
import vectorwave_amd as vw
from vectorwave_amd import _native as nat

import energy_restatement as ER
import fin_restatement as FR
import footprint_cases as F
import guarded
import host_calls as H
import mra_restatement as MR
import restatement_bi as RB
import restatement_generic as G

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32}
MODES = {F.EXACT: "exact", F.FMA: "fma"}


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    w = guarded.word_type(got.dtype)
    bad = np.flatnonzero(got.view(w).reshape(-1) != want.view(w).reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} elements differ from the reference, first at flat index "
                           f"{int(bad[0])}: {got.reshape(-1)[bad[0]]!r} vs {want.reshape(-1)[bad[0]]!r}")


def no_sentinel(*arrays):
    """No reference output used here contains the sentinel (asserted on the CPU, once per reference)."""
    for a in arrays:
        assert not guarded.holds_sentinel(a)


def analysis(w):
    return list(w.lowPassDecomposition()), list(w.highPassDecomposition())


def synthesis(w):
    return list(w.lowPassReconstruction()), list(w.highPassReconstruction())


def oracle_core(boundary, N):
    """oracle.decompose's mode, as tests/test_gpu_energy.py chooses it: MultiLevelMODWTTransform.decompose (core=True)
    except PERIODIC at N >= 1024, where the reference sends some levels through an FFT that the engine replaces by
    the direct sum; there the oracle's direct PERIODIC loops (core=False: BatchMODWT, no FFT, no cap) are the
    restatement."""
    return not (boundary == O.PERIODIC and N >= 1024)


def oracle_decompose(x, lo, hi, boundary, J):
    rows = [O.decompose(r, lo, hi, boundary, J, core=oracle_core(boundary, x.shape[1])) for r in x]
    return np.stack([r[0] for r in rows], axis=1), np.stack([r[1] for r in rows])


@functools.lru_cache(maxsize=None)
def forward_ref(wavelet, dtype, B, N, ld, J, boundary, fma):
    """(x [B, N], details, approx): the restatement of the forward of the rows H.rows lays out at `ld`."""
    w = F.bank(wavelet)
    x = guarded.row_matrix(H.rows(B, N, NP[dtype], ld), B, N, ld)
    lo, hi = analysis(w)
    if dtype == "f64" and not fma and len(lo) == len(hi):
        det, app = oracle_decompose(x, lo, hi, boundary, J)
    else:
        dec = G.decompose if len(lo) == len(hi) else RB.decompose
        det, app = dec(x, lo, hi, boundary, J, dtype=NP[dtype], fma=fma)
    no_sentinel(det, app)
    return frozen(x, np.ascontiguousarray(det), np.ascontiguousarray(app))


@functools.lru_cache(maxsize=None)
def inverse_ref(wavelet, dtype, B, N, J, boundary, fma, mask=0xFFFFFFFF, az=False):
    """(details, approx, y): the EXACT restatement's coefficients of fill_uniform rows, and their reconstruction."""
    w = F.bank(wavelet)
    _, det, app = forward_ref(wavelet, dtype, B, N, N, J, boundary, False)
    lo, hi = synthesis(w)
    if dtype == "f64" and not fma and len(lo) == len(hi):
        y = np.stack([O.reconstruct(det[:, b], app[b], lo, hi, boundary, w.wavelet_id, mask, az) for b in range(B)])
    else:
        rec = G.reconstruct if len(lo) == len(hi) else RB.reconstruct
        y = rec(det, app, lo, hi, boundary, w.wavelet_id, mask, az, dtype=NP[dtype], fma=fma)
    no_sentinel(y)
    return det, app, frozen(np.ascontiguousarray(y))


class Timing:
    """Launch counts per family of the calls made inside the block."""

    def __init__(self, engine):
        self.engine = engine

    def __enter__(self):
        self.engine.reset_timing()
        self.engine.enable_timing(True)
        return self

    def count(self, family):
        return self.engine.kernel_time(family)[1]

    def __exit__(self, *exc):
        self.engine.enable_timing(False)
        self.engine.reset_timing()


OTHER = {"forward": "forward_level", "forward_level": "forward", "inverse": "inverse_level", "inverse_level": "inverse"}


def call(engine, case, mode, pattern, B=None, **kw):
    """One guarded call of the case -> (side, results)."""
    import torch
    engine.bind_torch_stream()
    side = guarded.GuardedSide(torch, case.N, case.shifts(pattern))
    fn = H.CALLS.get(case.entry) or H.MORE_CALLS[case.entry]
    args = dict(case.extra, **kw)
    if case.ld:
        args["ld"] = case.ld
    with engine.options(**dict(case.opts)), Timing(engine) as t:
        st = fn(engine.lib, engine.ctx, side, B or case.B, case.N, case.J, case.boundary, w=F.bank(case.wavelet),
                flags=case.flags | mode, **args)
        assert st == 0, (case.id, pattern, MODES[mode], st, nat.last_error())
        torch.cuda.synchronize()
        if case.family:
            ran, other = t.count(case.family), t.count(OTHER[case.family])
            assert ran >= 1 and other == 0, (case.id, pattern, case.family, ran, other)
        if case.flags & nat.FLAG_REF_NONFINITE:
            # (the fix-up ran: over the rows a probing kernel flagged, or behind its own scan of the planes)
            assert t.count("ref_nonfinite") + t.count("ref_nonfinite_scan") == 1, (case.id, pattern)
    guarded.check(side)
    assert [a.name for a in side.arenas if not a.table] == list(case.pointers), (case.id, [a.name for a in side.arenas])
    out = side.results()
    side.close(engine.lib)
    return side, out


# ---- forward --------------------------------------------------------------------------------------------------------
SMALL = [c for c in F.FORWARD if c.id.startswith("fwd-small")]
LARGE = [c for c in F.FORWARD if not c.id.startswith("fwd-small") and c.B > 0]


def _forward(engine, case, mode, B=None):
    B = B or case.B
    x, det, app = forward_ref(case.wavelet, case.dtype, B, case.N, case.ld, case.J, case.boundary, mode == F.FMA)
    for pattern in case.shift_patterns():
        side, (got_d, got_a) = call(engine, case, mode, pattern, B=B)
        same_bits(side.matrices[0], x, "the rows the reference saw")
        same_bits(got_d, det, f"{case.id} {MODES[mode]} [{pattern}] details")
        same_bits(got_a, app, f"{case.id} {MODES[mode]} [{pattern}] approx")


@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES.values()))
@pytest.mark.parametrize("chunk", range(6))
def test_forward_small_rows(engine, chunk, mode):
    """k_forward_fused at N = 64, 67, 258: three boundaries, ldx = N, N + 3, N + 8, fp64 and fp32, and the validating
    and fix-up forms of each (NaN pads and guards: VW_OK, nothing flagged, no row recomputed)."""
    for case in SMALL[chunk::6]:
        _forward(engine, case, mode)


def pairs(cases):
    """(case, mode) for every accumulation mode the case's form exists in."""
    return [pytest.param(c, m, id=f"{c.id}-{MODES[m]}") for c in cases for m in c.modes]


@pytest.mark.parametrize("case,mode", pairs(LARGE))
def test_forward_forms(engine, case, mode):
    _forward(engine, case, mode)


@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES.values()))
def test_forward_persist_more_rows_than_workgroups(engine, mode):
    """N = 512, B = 2 x resident grid + 5 (the grid taken as tests/test_gpu_pair_keep.py takes it): every workgroup
    walks two or three rows, so the prefetch of the next row runs, and after the last row it must not."""
    import torch
    case = next(c for c in F.FORWARD if c.id == "fwd-persist-rows")
    per_cu = engine.roundtrip_occupancy(case.N, 8, case.J, mode)
    assert per_cu >= 1
    B = 2 * per_cu * torch.cuda.get_device_properties(0).multi_processor_count + 5
    _forward(engine, case, mode, B=B)


# ---- inverse --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", pairs(F.INVERSE))
def test_inverse_forms(engine, case, mode):
    fma = mode == F.FMA
    extra = dict(case.extra)
    if case.entry == "vw_modwt1_inverse_f64":
        w = F.bank(case.wavelet)
        _, det, app = forward_ref(case.wavelet, "f64", case.B, case.N, case.N, 1, case.boundary, False)
        if fma:
            want = RB.inverse1(app, det[0], *synthesis(w), case.boundary, fma=True)
        else:
            want = np.stack([O.modwt_inverse(app[b], det[0, b], *synthesis(w), case.boundary) for b in range(case.B)])
        no_sentinel(want)
        kw = dict(app=app, det=det[0])
    else:
        det, app, want = inverse_ref(case.wavelet, case.dtype, case.B, case.N, case.J, case.boundary, fma,
                                     extra.get("detail_mask", 0xFFFFFFFF), bool(extra.get("approx_zero", 0)))
        kw = dict(det=det) if extra.get("app", None) is False else dict(det=det, app=app)
    for pattern in case.shift_patterns():
        _, (y,) = call(engine, case, mode, pattern, **kw)
        same_bits(y, want, f"{case.id} {MODES[mode]} [{pattern}] y")


# ---- the same call on plain tensors ---------------------------------------------------------------------------------
def plain(engine, fn, *args, opts=(), **kw):
    """The results of the builder on tests/host_calls.py's plain device Side: torch's own aligned allocations, finite
    padding.  What a form without a bit-exact restatement must equal on guarded, shifted, NaN-padded arenas."""
    import torch
    engine.bind_torch_stream()
    side = H.Side(torch)
    with engine.options(**dict(opts)):
        assert fn(engine.lib, engine.ctx, side, *args, **kw) == 0, nat.last_error()
    out = side.results()
    side.close(engine.lib)
    return out


def guarded_runs(engine, fn, N, pointers, *args, opts=(), patterns=None, **kw):
    """The builder on guarded arenas under every shift pattern: yields (pattern, side, results), checked."""
    import torch
    engine.bind_torch_stream()
    for pattern in patterns or ("none", "all") + tuple(pointers):
        side = guarded.GuardedSide(torch, N, pattern if pattern in ("none", "all") else {pointers.index(pattern)})
        with engine.options(**dict(opts)), Timing(engine) as t:
            st = fn(engine.lib, engine.ctx, side, *args, **kw)
            assert st == 0, (pattern, st, nat.last_error())
            torch.cuda.synchronize()
            side.launches = {f: t.count(f) for f in ("forward", "forward_level", "inverse", "inverse_level", "mra",
                                                     "energy_fused", "energy_tree", "ref_nonfinite")}
        guarded.check(side)
        assert [a.name for a in side.arenas if not a.table] == list(pointers), [a.name for a in side.arenas]
        out = side.results()
        side.close(engine.lib)
        yield pattern, side, out


def all_same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        same_bits(g, np.asarray(w).reshape(np.shape(g)), f"{what} output {k}")


# ---- streaming history ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,J", [(8192, 4), (48, 2)])
def test_stream_blocks_and_flush(engine, N, J):
    """vw_stream_process_f64, ZERO_PADDING: two blocks (the second reads the history the first left), then
    vw_stream_flush_f64 -- EXACT against the oracle's StreamRestatement, FMA against the same calls on plain tensors."""
    import torch
    B, w = 3, F.bank("db4")
    lo, hi = analysis(w)
    blocks = [O.fill_uniform(B * N, 42, offset=k * B * N).reshape(B, N) for k in range(2)]
    tail = min(7, N)
    refs = [O.StreamRestatement(lo, hi, O.ZERO_PADDING, J) for _ in range(B)]
    want = [[r.process(blk[b]) for b, r in enumerate(refs)] for blk in blocks] + [[r.flush(tail) for r in refs]]
    want = [(np.stack([d for d, _ in step], axis=1), np.stack([a for _, a in step])) for step in want]
    no_sentinel(*[a for step in want for a in step])
    engine.bind_torch_stream()
    lib = engine.lib

    def run(make_side, mode):
        h = c_void_p()
        keep = make_side()
        assert lib.vw_stream_create(engine.ctx, keep.table(lo), keep.table(hi), len(lo), nat.ZERO_PADDING, J,
                                    byref(h)) == 0, nat.last_error()
        out = []
        try:
            for k in range(3):
                s = make_side()
                n = N if k < 2 else tail
                if k < 2:
                    st = lib.vw_stream_process_f64(h, s.inp(blocks[k], name="block"), B, N, s.flags | mode,
                                                   s.out((J, B, n), name="details"), s.out((B, n), name="approx"))
                else:
                    st = lib.vw_stream_flush_f64(h, tail, s.flags | mode, s.out((J, B, n), name="details"),
                                                 s.out((B, n), name="approx"))
                assert st == 0, (k, st, nat.last_error())
                torch.cuda.synchronize()
                if isinstance(s, guarded.GuardedSide):
                    guarded.check(s)
                out.append(s.results())
        finally:
            assert lib.vw_stream_destroy(h) == 0
        return out

    for mode in MODES:
        base = run(lambda: H.Side(torch), mode) if mode == F.FMA else want
        for shifts in ("none", "all", {0}, {1}, {2}):
            got = run(lambda: guarded.GuardedSide(torch, N, shifts), mode)
            for k in range(3):
                all_same(got[k], base[k], f"stream N={N} {MODES[mode]} shifts={shifts} step {k}")


# ---- fused thresholds -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4096, 129])
@pytest.mark.parametrize("name", ["swt", "universal", "sure"])
def test_denoise(engine, name, N):
    """vw_swt_denoise_f64 / vw_wavelet_denoise_f64 (the inverse reads its thresholds from the workspace): rows at
    ldx = N + 3.  EXACT: y and the thresholds are the oracle's; FMA: the same call on plain tensors."""
    B, J, ld, w = 3, 3, N + 3, F.bank("db4")
    lo, hi = analysis(w)
    x = guarded.row_matrix(H.rows(B, N, np.float64, ld), B, N, ld)
    if name == "swt":
        fn, kw = H.swt_denoise, {}
        ref = [O.swt_denoise(x[b], lo, hi, O.PERIODIC, J, -1.0, True, wavelet_id=w.wavelet_id) for b in range(B)]
        want = [np.stack([y for y, _ in ref]), np.array([t for _, t in ref])]
    else:
        method = O.UNIVERSAL if name == "universal" else O.SURE
        fn, kw = H.wavelet_denoise, dict(method=method)
        ref = [O.wavelet_denoise(x[b], lo, hi, O.PERIODIC, J, method, wavelet_id=w.wavelet_id) for b in range(B)]
        want = [np.stack([y for y, _ in ref]), np.stack([t for _, t in ref], axis=1)]
    no_sentinel(*want)
    for mode in MODES:
        base = plain(engine, fn, B, N, J, nat.PERIODIC, ld=ld, flags=mode, **kw) if mode == F.FMA else want
        for pattern, side, got in guarded_runs(engine, fn, N, ("x", "y", "thresholds"), B, N, J, nat.PERIODIC, ld=ld,
                                               flags=mode, **kw):
            all_same(got, base, f"{name} N={N} {MODES[mode]} [{pattern}]")


# ---- round trip -----------------------------------------------------------------------------------------------------
def _roundtrip_ref(N, J, B, fma):
    w = F.bank("db4")
    x = O.fill_uniform(B * N, 42).reshape(B, N)
    if fma:
        det, app = G.decompose(x, *analysis(w), O.PERIODIC, J, fma=True)
        y = G.reconstruct(det, app, *synthesis(w), O.PERIODIC, w.wavelet_id, fma=True)
    else:
        det, app = oracle_decompose(x, *analysis(w), O.PERIODIC, J)
        y = np.stack([O.reconstruct(det[:, b], app[b], *synthesis(w), O.PERIODIC, w.wavelet_id) for b in range(B)])
    no_sentinel(det, app, y)
    return x, [np.ascontiguousarray(det), app, y]


def roundtrip_call(lib, ctx, s, B, N, J, bd, flags=0):
    w = F.bank("db4")
    x = O.fill_uniform(B * N, 42).reshape(B, N)
    lo, hi = (s.table(t) for t in analysis(w))
    rlo, rhi = (s.table(t) for t in synthesis(w))
    return lib.vw_modwt_roundtrip_f64(ctx, s.inp(x, name="x"), B, N, N, lo, hi, rlo, rhi, 8, w.wavelet_id, bd, J,
                                      s.flags | flags, s.out((J, B, N), name="details"), s.out((B, N), name="approx"),
                                      s.out((B, N), name="y"))


@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES.values()))
@pytest.mark.parametrize("N,J", [(512, 3), (4096, 4)])
def test_roundtrip_call(engine, N, J, mode):
    """vw_modwt_roundtrip_f64: x, details, approx and y in arenas, against forward followed by inverse."""
    B = 3
    _, want = _roundtrip_ref(N, J, B, mode == F.FMA)
    for pattern, side, got in guarded_runs(engine, roundtrip_call, N, ("x", "details", "approx", "y"), B, N, J,
                                           nat.PERIODIC, flags=mode):
        all_same(got, want, f"roundtrip N={N} J={J} {MODES[mode]} [{pattern}]")


@pytest.fixture(scope="module")
def keep_ctxs():
    """A context per forced VW_PAIR_KEEP, each on a stream of its own (a capture needs a non-default stream)."""
    import torch
    made = {}
    for k in (0, 1, 2):
        e = vw.Engine(0)
        e.set_option("VW_PAIR_FUSE", 1)
        e.set_option("VW_PAIR_KEEP", k)
        made[k] = (e, torch.cuda.Stream())
    yield made
    torch.cuda.synchronize()
    for e, _ in made.values():
        e.close()


def _captured_pair(eng, stream, N, J, B, mode, shifts):
    """A captured forward followed by its inverse, all five arrays (x, details, approx, y; the details and the
    approximation are both outputs of the forward and inputs of the inverse) in arenas; replayed twice, checked after
    each replay.  -> (fused pairs, [results of replay 1, of replay 2])."""
    import torch
    w = F.bank("db4")
    lib, ctx = eng.lib, eng.ctx
    with torch.cuda.stream(stream):
        eng.bind_torch_stream()
        s = guarded.GuardedSide(torch, N, shifts)
        lo, hi = (s.table(t) for t in analysis(w))
        rlo, rhi = (s.table(t) for t in synthesis(w))
        px = s.inp(O.fill_uniform(B * N, 42).reshape(B, N), name="x")
        pd, pa, py = s.out((J, B, N), name="details"), s.out((B, N), name="approx"), s.out((B, N), name="y")

        def step():
            assert lib.vw_modwt_forward_f64(ctx, px, B, N, N, lo, hi, 8, w.wavelet_id, nat.PERIODIC, J, mode, pd,
                                            pa) == 0, nat.last_error()
            assert lib.vw_modwt_inverse_f64(ctx, pd, pa, B, N, rlo, rhi, 8, w.wavelet_id, nat.PERIODIC, J, 0xFFFFFFFF, 0,
                                            mode, py) == 0, nat.last_error()

        step()  # outside any capture first, as tests/test_gpu_pair_keep.py does
        torch.cuda.synchronize()
        guarded.check(s)
        g = eng.capture(step)
        _, fused = g.stats()
        outs = []
        for _ in range(2):
            for a in s.arenas:  # back to the sentinel: every replay must write everything again
                if a.kind == "out":
                    a.store.copy_(torch.from_numpy(a.orig.view(np.int64)))
            g.launch(1)
            torch.cuda.synchronize()
            guarded.check(s)
            outs.append(s.results())
        g.close()
    return fused, outs


@pytest.mark.parametrize("keep", [0, 1, 2])
@pytest.mark.parametrize("N", [512, 4096])
def test_captured_pair(keep_ctxs, keep, N):
    """engine.capture of forward -> inverse under VW_PAIR_KEEP = 0, 1, 2 at J = keep + 2 (exactly one reload) and the
    row's deepest level: one k_roundtrip launch when every pointer is aligned (fused_pairs == 1, the forced variant
    is the one vw_roundtrip_variant reports), two kernels when a pointer is shifted (fused_pairs == 0)."""
    eng, stream = keep_ctxs[keep]
    B = 3
    for J in sorted({keep + 2, vw.max_levels(N, 8)}):
        for mode in MODES:
            k, per_cu = eng.roundtrip_variant(N, 8, J, mode)
            assert k == keep and per_cu >= 1, (keep, k, per_cu)
            _, want = _roundtrip_ref(N, J, B, mode == F.FMA)
            for shifts in ("none", "all", {0}, {1}, {2}, {3}):
                fused, outs = _captured_pair(eng, stream, N, J, B, mode, shifts)
                assert fused == (1 if shifts == "none" else 0), (keep, N, J, mode, shifts, fused)
                for r, got in enumerate(outs):
                    all_same(got, want, f"captured pair KEEP={keep} N={N} J={J} {MODES[mode]} shifts={shifts} replay {r}")


@pytest.mark.parametrize("keep,J", [(2, 4), (1, 3), (0, 2)])
def test_captured_pair_more_rows_than_workgroups(keep_ctxs, keep, J):
    """N = 512, B = 2 x resident grid + 5: the round-trip kernel's prefetch of the next row, and its last row (EXACT:
    the oracle restates thousands of rows quickly; FMA runs at B = 3 above)."""
    import torch
    eng, stream = keep_ctxs[keep]
    mode = F.EXACT
    per_cu = eng.roundtrip_occupancy(512, 8, J, mode)
    assert per_cu == eng.roundtrip_variant(512, 8, J, mode)[1] and per_cu >= 1
    B = 2 * per_cu * torch.cuda.get_device_properties(0).multi_processor_count + 5
    _, want = _roundtrip_ref(512, J, B, mode == F.FMA)
    for shifts in ("none", "all"):
        fused, outs = _captured_pair(eng, stream, 512, J, B, mode, shifts)
        assert fused == (1 if shifts == "none" else 0)
        for r, got in enumerate(outs):
            all_same(got, want, f"captured pair KEEP={keep} B={B} shifts={shifts} replay {r}")


# ---- the other families -----------------------------------------------------------------------------------------------
# tests/host_calls.py's B = 3, J = 2 at its N = 48, at one odd N and at one above 1024.
SHAPES = [48, 129, 4100]
B3, J2 = 3, 2


@pytest.mark.parametrize("fused", [0, 2])
@pytest.mark.parametrize("N", SHAPES)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mra(engine, dtype, N, fused):
    """vw_mra_planes_* on random coefficient planes and vw_modwt_mra_* on padded rows, VW_MRA_FUSED = 0 (the J + 1
    masked inverses) and 2 (k_mra wherever it fits), against tests/mra_restatement.py in both accumulation modes."""
    w, dt = F.bank("db4"), NP[dtype]
    opts = (("VW_MRA_FUSED", fused),)
    det, app = H.u(J2 * B3 * N, dt).reshape(J2, B3, N), H.u(B3 * N, dt).reshape(B3, N)
    ld = N + 3
    x = guarded.row_matrix(H.rows(B3, N, dt, ld), B3, N, ld)
    for mode in MODES:
        fma = mode == F.FMA
        want = MR.mra(det, app, *synthesis(w), O.PERIODIC, w.wavelet_id, dt, fma)
        no_sentinel(want)
        fn = H.mra_planes if dtype == "f64" else H.MORE_CALLS["vw_mra_planes_f32"]
        for pattern, side, got in guarded_runs(engine, fn, N, ("details", "approx", "out"), B3, N, J2, nat.PERIODIC,
                                               opts=opts, flags=mode):
            all_same(got, [want], f"mra_planes {dtype} N={N} fused={fused} {MODES[mode]} [{pattern}]")
            if fused == 0:
                assert side.launches["mra"] == 0 and side.launches["inverse"] + side.launches["inverse_level"] >= 1
            elif pattern == "none":
                assert side.launches["mra"] >= 1, side.launches
        fd, fa = G.decompose(x, *analysis(w), O.PERIODIC, J2, dtype=dt, fma=fma)
        want = MR.mra(fd, fa, *synthesis(w), O.PERIODIC, w.wavelet_id, dt, fma)
        fn = H.modwt_mra if dtype == "f64" else H.MORE_CALLS["vw_modwt_mra_f32"]
        for pattern, side, got in guarded_runs(engine, fn, N, ("x", "out"), B3, N, J2, nat.PERIODIC, opts=opts, ld=ld,
                                               flags=mode):
            all_same(got, [want], f"modwt_mra {dtype} N={N} fused={fused} {MODES[mode]} [{pattern}]")


def _tree_bound(ref, N):  # tests/test_gpu_energy.py's bar for VW_FLAG_TREE_SUMS, by reference: N * 2^-52 * E_seq
    return N * 2.0 ** -52 * ref


@pytest.mark.parametrize("N", SHAPES)
@pytest.mark.parametrize("form", ["default", "tree", "unfused"])
def test_energy(engine, form, N):
    """vw_modwt_energy_f64 on padded rows: the default, VW_FLAG_TREE_SUMS and VW_ENERGY_FUSED = 0.  The sequential
    EXACT forms are tests/energy_restatement.py's bits; tree sums keep tests/test_gpu_energy.py's reordering bound and,
    as every FMA form, must be the bits of the same call on plain tensors: tree order must not depend on alignment."""
    w, ld = F.bank("db4"), N + 3
    lo, hi = analysis(w)
    x = guarded.row_matrix(H.rows(B3, N, np.float64, ld), B3, N, ld)
    seq = ER.energies(x, lo, hi, O.PERIODIC, J2, core=oracle_core(O.PERIODIC, N))
    no_sentinel(seq)
    flags = nat.FLAG_TREE_SUMS if form == "tree" else 0
    opts = (("VW_ENERGY_FUSED", 0),) if form == "unfused" else ()
    for mode in MODES:
        exact = mode == F.EXACT and form != "tree"
        base = [seq] if exact else plain(engine, H.energy, B3, N, J2, nat.PERIODIC, opts=opts, ld=ld, flags=flags | mode)
        for pattern, side, got in guarded_runs(engine, H.energy, N, ("x", "energies"), B3, N, J2, nat.PERIODIC,
                                               opts=opts, ld=ld, flags=flags | mode):
            all_same(got, base, f"energy {form} N={N} {MODES[mode]} [{pattern}]")
            if form == "tree" and mode == F.EXACT:
                assert (np.abs(got[0] - seq) <= _tree_bound(seq, N)).all()
            if form == "unfused":
                assert side.launches["energy_fused"] == 0, side.launches
            if form == "tree":
                assert side.launches["energy_fused"] + side.launches["energy_tree"] >= 1, side.launches


@pytest.mark.parametrize("N", SHAPES)
def test_energy_planes(engine, N):
    det, app = H.u(J2 * B3 * N).reshape(J2, B3, N), H.u(B3 * N).reshape(B3, N)
    seq = ER.planes_energies(det, app)
    no_sentinel(seq)
    for flags in (0, nat.FLAG_TREE_SUMS):
        base = [seq] if not flags else plain(engine, H.energy_planes, B3, N, J2, nat.PERIODIC, flags=flags)
        for pattern, side, got in guarded_runs(engine, H.energy_planes, N, ("details", "approx", "energies"), B3, N, J2,
                                               nat.PERIODIC, flags=flags):
            all_same(got, base, f"energy_planes N={N} flags={flags} [{pattern}]")
            if flags:
                assert (np.abs(got[0] - seq) <= _tree_bound(seq, N)).all()


def cwt_call(t, dtype):
    """vw_cwt_*: Morlet tables of vectorwave_amd.cwt.build_tables; the scale descriptors, both tap tables (host
    arrays) and the rows guarded."""
    def call(lib, ctx, s, B, N, J, bd, ld=None, flags=0):
        desc = (nat.CwtScale * len(t.scales))(*[nat.CwtScale(int(a), int(k), int(o), float(q)) for a, k, o, q in t.scales])
        keep = getattr(s, "keep", None)
        if hasattr(s, "structs"):
            from ctypes import POINTER, cast
            dp = cast(c_void_p(s.structs(desc, name="scales")), POINTER(nat.CwtScale))
        else:
            keep.append(desc)
            dp = desc
        S = len(t.scales)
        fn = lib.vw_cwt_f64 if dtype == np.float64 else lib.vw_cwt_f32
        return fn(ctx, s.rows(B, N, ld, dtype, name="x"), B, N, ld, dp, S, s.table(t.taps_re, "taps_re"),
                  s.table(t.taps_im, "taps_im"), t.taps_re.size, t.ext, t.wrap, s.flags | flags,
                  s.out((B, S, N), dtype, name="out_re"), s.out((B, S, N), dtype, name="out_im"))
    return call


@pytest.mark.parametrize("N", [31, 1000])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cwt(engine, dtype, N):
    """vw_cwt_*: Morlet at scales 0.5 (the support clamp), 7 and 150 (wider than the row), rows at ldx = N + 3.  EXACT:
    tests/cwt_restatement.py's bits.  FMA: the bits of the same call on plain tensors, within tests/test_gpu_cwt.py's
    derived bound (cwt_restatement.fma_bound) of the EXACT restatement."""
    import cwt_restatement as CR
    from vectorwave_amd.cwt import CWTConfig, MorletWavelet, PaddingStrategy, build_tables
    dt, ld = NP[dtype], N + 3
    t = build_tables(MorletWavelet(), CWTConfig(paddingStrategy=PaddingStrategy.REFLECT, fftEnabled=False),
                     [0.5, 7.0, 150.0], N)
    x = guarded.row_matrix(H.rows(B3, N, dt, ld), B3, N, ld)
    rows = [CR.correlate(x[b], N, t.scales, t.taps_re, t.taps_im, t.ext, t.wrap, dt) for b in range(B3)]
    want = [np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])]
    no_sentinel(*want)
    fn = cwt_call(t, dt)
    for mode in MODES:
        base = want if mode == F.EXACT else plain(engine, fn, B3, N, 0, 0, ld=ld, flags=mode)
        if mode == F.FMA:
            bounds = CR.fma_bound(t.scales, t.taps_re, t.taps_im, float(np.max(np.abs(x))), dt)
            for b, bound, ref in zip(base, bounds, want):
                diff = np.max(np.abs(b.astype(np.float64) - ref.astype(np.float64)), axis=(0, 2))
                assert np.all(diff <= bound), (diff, bound)
        for pattern, side, got in guarded_runs(engine, fn, N, ("x", "out_re", "out_im"), B3, N, 0, 0, ld=ld, flags=mode):
            all_same(got, base, f"cwt {dtype} N={N} {MODES[mode]} [{pattern}]")


@pytest.mark.parametrize("N", SHAPES)
def test_fin(engine, N):
    """vw_fin_analyze_f64, vw_fin_sharpe_f64, vw_fin_wavelet_sharpe_f64 on padded rows, against
    tests/fin_restatement.py."""
    w, ld = F.bank("db4"), N + 3
    lo, hi = analysis(w)
    x = guarded.row_matrix(H.rows(B3, N, np.float64, ld), B3, N, ld)
    cases = [(H.fin_analyze, ("prices", "out"), FR.analyze_batch(x + 2.0, lo, hi, 3.0)),
             (H.fin_sharpe, ("returns", "out"), np.array([FR.sharpe(r, 0.01) for r in x])),
             (H.fin_wavelet_sharpe, ("returns", "out"),
              np.array([FR.wavelet_sharpe(r, lo, hi, O.PERIODIC, 0.01) for r in x]))]
    for fn, pointers, want in cases:
        no_sentinel(want)
        for pattern, side, got in guarded_runs(engine, fn, N, pointers, B3, N, J2, nat.PERIODIC, ld=ld):
            all_same(got, [want], f"{fn.__name__} N={N} [{pattern}]")


def median_call(center):
    def call(lib, ctx, s, B, N, J, bd, flags=0):
        x = np.stack([O.java_random_signal(N, 5 + b) for b in range(B)])
        cp = s.inp(np.array(center[:B]), name="center") if center is not None else None
        xp = s.inp(x, name="x")
        return lib.vw_median_f64(ctx, xp, B, N, cp, s.flags | flags, s.out((B,), name="median"))
    return call


@pytest.mark.parametrize("N", [129, 4096, 20000])
def test_sigma_and_median(engine, N):
    """vw_noise_sigma_f64 and vw_median_f64 (with and without a center; rows above 16384 with a center go through the
    per-context scratch buffer): the oracle's values."""
    x = H.u(B3 * N).reshape(B3, N)
    want = np.array([O.noise_sigma(r) for r in x])
    for pattern, side, got in guarded_runs(engine, H.noise_sigma, N, ("coeffs", "sigma"), B3, N, J2, 0):
        all_same(got, [want], f"noise_sigma N={N} [{pattern}]")
    xm = np.stack([O.java_random_signal(N, 5 + b) for b in range(B3)])
    center = [0.1, -0.25, 0.0]
    for c, pointers in ((None, ("x", "median")), (center, ("center", "x", "median"))):
        want = np.array([O.java_median(np.abs(xm[b] - (c[b] if c else 0.0))) for b in range(B3)])
        for pattern, side, got in guarded_runs(engine, median_call(c), N, pointers, B3, N, 0, 0):
            all_same(got, [want], f"median N={N} center={c is not None} [{pattern}]")


@pytest.mark.parametrize("N", SHAPES)
def test_threshold_in_place(engine, N):
    x = H.u(B3 * N).reshape(B3, N)
    want = np.stack([O.threshold(r, 0.25, True) for r in x]).reshape(-1)
    for pattern, side, got in guarded_runs(engine, H.threshold, N, ("c", "thr"), B3, N, J2, 0):
        all_same(got, [want], f"threshold N={N} [{pattern}]")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("rows,cols", [(3, 48), (65, 130)])
def test_transpose(engine, rows, cols, dtype):
    want = H.u(rows * cols, NP[dtype]).reshape(rows, cols).T
    fn = H.transpose if dtype == "f64" else H.MORE_CALLS["vw_transpose_f32"]
    for pattern, side, got in guarded_runs(engine, fn, cols, ("in", "out"), rows, cols, 0, 0):
        all_same(got, [np.ascontiguousarray(want)], f"transpose {rows}x{cols} {dtype} [{pattern}]")


def test_window_gather_abs(engine):
    """vw_window_gather_abs_f64: count < wsize and a start that wraps; the window is written at (start + k) % wsize
    only, every other element keeps its bits."""
    n, wsize, start = 257, 11, 8
    src = O.java_random_signal(n, 3)
    idx = np.array([5, 256, 0, 77, 130, 131], dtype=np.int32)
    window = O.java_random_signal(wsize, 4)
    want = window.copy()
    for k, i in enumerate(idx):
        want[(start + k) % wsize] = abs(src[i])

    def call(lib, ctx, s, *_):
        ia = guarded.Arena("idx", "in", idx, 0, n, None)   # a host array: guarded, never shifted
        ia.table = True
        s.arenas.append(ia)
        return lib.vw_window_gather_abs_f64(ctx, s.inp(src, name="src"), c_void_p(ia.ptr), len(idx),
                                            s.inout(window, name="window"), wsize, start)

    for pattern, side, got in guarded_runs(engine, call, n, ("src", "window")):
        all_same(got, [want], f"window_gather_abs [{pattern}]")


@pytest.mark.parametrize("N", [2, 129, 4100])
def test_stddev(engine, N):
    x = O.java_random_signal(N, 9)
    want = np.array([O.java_std_guarded(x)])

    def call(lib, ctx, s, *_):
        return lib.vw_stddev_f64(ctx, s.inp(x, name="x"), N, s.flags, s.out((1,), name="out"))

    for pattern, side, got in guarded_runs(engine, call, N, ("x", "out")):
        all_same(got, [want], f"stddev N={N} [{pattern}]")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("count", [1, 255, 4097])
def test_fill_uniform(engine, count, dtype):
    want = O.fill_uniform(count, 77, offset=13).astype(NP[dtype])

    def call(lib, ctx, s, *_):
        fn = lib.vw_fill_uniform_f64 if dtype == "f64" else lib.vw_fill_uniform_f32
        return fn(ctx, s.out((count,), NP[dtype], name="x"), count, 77, 13)

    for pattern, side, got in guarded_runs(engine, call, count, ("x",)):
        all_same(got, [want], f"fill_uniform {count} {dtype} [{pattern}]")
