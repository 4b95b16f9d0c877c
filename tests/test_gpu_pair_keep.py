"""VW_PAIR_KEEP: the round-trip kernel keeps 0, 1 or 2 detail planes below d_J in registers instead of reading them back.

Four contexts, each on a stream of its own: VW_PAIR_KEEP = 0, 1 and 2 forced, and VW_PAIR_FUSE = 0 (the two separate
kernels), whose capture is the reference -- computed once per case and shared by the three variants.  Before any
comparison vw_roundtrip_variant must report that the forced variant is the one the context launches.  details, approx
and y are pre-filled with NaN and compared byte for byte, over two replays of the graph.

Shapes are the smallest at which each mechanism can go wrong.  Waves: N = 512 (one wave per workgroup), 1024, and
4096 (8 waves, the headline's workgroup; db4 only); 2, 4, 6 and 8 taps; EXACT and FMA.  Levels for KEEP = k: J = 1 and
J = k + 1 (nothing but registers, no reload and no vmcnt(0)), J = k + 2 (exactly one reload: the counted wait sits
directly before the only load), J = k + 3 and the row's deepest level (the waited reload is followed by vmcnt(0)
ones); B = 1 and 3.  More rows than resident workgroups (N = 512, B = 2 x resident grid + 5): the DMA-issued and the
no-next-row branch of the counted wait both run, with J odd and even since the buffer the next row lands in alternates.
"""
from ctypes import c_void_p

import numpy as np
import pytest

from oracle import oracle as O
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import Daubechies, Haar, Symlet

import restatement_generic as G

pytestmark = pytest.mark.gpu

K = 2  # forward -> inverse pairs per capture
KEEPS = (0, 1, 2)
# haar, db2, db3, db4: 2, 4, 6 and 8 taps (sym3: the catalogue's six-tap Daubechies-3)
WAVELETS = [Haar.INSTANCE, Daubechies.DB2, Symlet.SYM3, Daubechies.DB4]


def lohi(w):
    return w.lowPassDecomposition(), w.highPassDecomposition()


def rlohi(w):
    return w.lowPassReconstruction(), w.highPassReconstruction()


@pytest.fixture(scope="module")
def ctxs(engine):
    """({k: (context with VW_PAIR_KEEP = k, stream)}, (context with VW_PAIR_FUSE = 0, stream))."""
    import torch
    keep = {}
    for k in KEEPS:
        e = vw.Engine(0)
        e.set_option("VW_PAIR_FUSE", 1)
        e.set_option("VW_PAIR_KEEP", k)
        keep[k] = (e, torch.cuda.Stream())
    off = vw.Engine(0)
    off.set_option("VW_PAIR_FUSE", 0)
    yield keep, (off, torch.cuda.Stream())
    torch.cuda.synchronize()
    for e, _ in keep.values():
        e.close()
    off.close()


def run(eng_stream, w, B, N, J, flags, steps=K, seed=7):
    """Capture `steps` forward -> inverse pairs on the context, replay the graph twice; (details, approx, y) of every
    step as numpy arrays, and the number of fused pairs vw_graph_stats reports."""
    import torch
    eng, stream = eng_stream
    lib, ctx = eng.lib, eng.ctx
    lo, hi = (nat.taps_array(t) for t in lohi(w))
    rlo, rhi = (nat.taps_array(t) for t in rlohi(w))
    L = len(lohi(w)[0])
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    with torch.cuda.stream(stream):
        eng.bind_torch_stream()
        x = torch.empty((steps, B, N), dtype=torch.float64, device="cuda")
        det = torch.empty((steps, J, B, N), dtype=torch.float64, device="cuda")
        app = torch.empty((steps, B, N), dtype=torch.float64, device="cuda")
        y = torch.empty((steps, B, N), dtype=torch.float64, device="cuda")

        def step(k):
            assert lib.vw_modwt_forward_f64(ctx, P(x[k]), B, N, N, lo, hi, L, w.wavelet_id, O.PERIODIC, J, flags,
                                            P(det[k]), P(app[k])) == 0, nat.last_error()
            assert lib.vw_modwt_inverse_f64(ctx, P(det[k]), P(app[k]), B, N, rlo, rhi, L, w.wavelet_id, O.PERIODIC, J,
                                            0xFFFFFFFF, 0, flags, P(y[k])) == 0, nat.last_error()

        eng.fill_uniform(x, seed)
        step(0)  # outside any capture: LDS limits and occupancies of every variant
        torch.cuda.synchronize()
        g = eng.capture(lambda: [step(k) for k in range(steps)])
        _, fused = g.stats()
        out = []
        for _ in range(2):  # a replay, then a second one: the same bytes
            eng.fill_uniform(x, seed)
            for t in (det, app, y):
                t.fill_(float("nan"))
            g.launch(1)
            torch.cuda.synchronize()
            out.append(tuple(t.cpu().numpy().copy() for t in (det, app, y)))
        g.close()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b, equal_nan=True), "a second replay of the graph gives other bytes"
    assert not any(np.isnan(a).any() for a in out[0]), "an output was not written"
    return out[0], fused


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def forced(ctxs, k, N, L, J, flags):
    """The context that forces variant k, after checking that this is what it launches for the shape."""
    keep, per_cu = ctxs[0][k][0].roundtrip_variant(N, L, J, flags)
    assert keep == k and per_cu >= 1, (k, keep, per_cu)
    return ctxs[0][k]


def levels_for(k, deepest):
    return {J for J in (1, k + 1, k + 2, k + 3, deepest) if J <= deepest}


CASES = [(w, N) for N in (512, 1024) for w in WAVELETS] + [(Daubechies.DB4, 4096)]


@pytest.mark.parametrize("w,N", CASES, ids=lambda v: v.name() if hasattr(v, "name") else str(v))
def test_every_variant_gives_the_unfused_bytes(ctxs, w, N):
    L = len(lohi(w)[0])
    deepest = vw.max_levels(N, L)
    compared = 0
    for J in sorted(set().union(*(levels_for(k, deepest) for k in KEEPS))):
        for flags in (0, nat.FLAG_FMA):
            for B in (1, 3):
                ref, fused0 = run(ctxs[1], w, B, N, J, flags)
                assert fused0 == 0
                for k in KEEPS:
                    if J not in levels_for(k, deepest):
                        continue
                    got, fused = run(forced(ctxs, k, N, L, J, flags), w, B, N, J, flags)
                    assert fused == K, (k, J, flags, B, fused)
                    assert same_bytes(got, ref), f"KEEP={k} J={J} flags={flags} B={B}: differs from the two kernels"
                    compared += 1
    print(f"  {w.name()} N={N}: {compared} captures compared, levels up to {deepest}")
    assert compared >= 2 * 2 * sum(len(levels_for(k, deepest)) for k in KEEPS)


# KEEP = 2: no reload, one, two; KEEP = 1: none, one; KEEP = 0 beside them at an odd and an even J
@pytest.mark.parametrize("k,J", [(2, 3), (2, 4), (2, 5), (1, 2), (1, 3), (0, 2), (0, 3)])
def test_more_rows_than_resident_workgroups(ctxs, k, J):
    """N = 512, B = twice the resident grid + 5: every workgroup walks two or three rows, so the wait ahead of the
    first reload runs behind an issued DMA and, on the last row, without one; with no reload the row loop's closing
    wait retires the DMA by itself."""
    import torch
    w = Daubechies.DB4
    flags = nat.FLAG_FMA if J % 2 else 0
    ctx = forced(ctxs, k, 512, 8, J, flags)
    per_cu = ctx[0].roundtrip_occupancy(512, 8, J, flags)
    assert per_cu == ctx[0].roundtrip_variant(512, 8, J, flags)[1] and per_cu >= 1
    B = 2 * per_cu * torch.cuda.get_device_properties(0).multi_processor_count + 5
    got, fused = run(ctx, w, B, 512, J, flags, steps=1)
    ref, fused0 = run(ctxs[1], w, B, 512, J, flags, steps=1)
    print(f"  KEEP={k} J={J}: {per_cu} workgroups per CU, B = {B}")
    assert fused == 1 and fused0 == 0
    assert same_bytes(got, ref)


@pytest.mark.parametrize("N", [512, 1024, 4096])
def test_uncaptured_roundtrip_call(ctxs, engine, N):
    """vw_modwt_roundtrip_f64 outside a capture, under each forced variant: the bytes of forward followed by inverse."""
    import torch
    off, off_stream = ctxs[1]
    for w in WAVELETS if N < 4096 else [Daubechies.DB4]:
        L = len(lohi(w)[0])
        deepest = vw.max_levels(N, L)
        for J in sorted({J for J in (1, 2, 3, 4, deepest) if J <= deepest}):
            for flags in (0, nat.FLAG_FMA):
                x = torch.empty((3, N), dtype=torch.float64, device="cuda")
                engine.fill_uniform(x, 11)
                torch.cuda.synchronize()
                with torch.cuda.stream(off_stream):
                    det0, app0 = off.forward(x, *lohi(w), w.wavelet_id, O.PERIODIC, J, flags)
                    y0 = off.inverse(det0, app0, *rlohi(w), w.wavelet_id, O.PERIODIC, J, flags)
                for k in KEEPS:
                    eng, stream = forced(ctxs, k, N, L, J, flags)
                    with torch.cuda.stream(stream):
                        det, app, y = eng.roundtrip(x, *lohi(w), *rlohi(w), w.wavelet_id, O.PERIODIC, J, flags)
                    torch.cuda.synchronize()
                    assert torch.equal(det, det0) and torch.equal(app, app0) and torch.equal(y, y0), \
                        (w.name(), k, J, flags)


@pytest.mark.parametrize("w", WAVELETS, ids=lambda w: w.name())
def test_exact_keep2_is_bit_exact_against_the_restatement(ctxs, w):
    """One case per wavelet: KEEP = 2, N = 1024 at its deepest level, three rows, EXACT."""
    N, L = 1024, len(lohi(w)[0])
    J = vw.max_levels(N, L)
    (det, app, y), fused = run(forced(ctxs, 2, N, L, J, 0), w, 3, N, J, 0, steps=1)
    assert fused == 1
    x = O.fill_uniform(3 * N, 7).reshape(3, N)
    for b in range(3):
        d_ref, a_ref = O.decompose(x[b], *lohi(w), O.PERIODIC, J, core=False)
        assert np.array_equal(det[0][:, b, :], d_ref), f"details row {b}"
        assert np.array_equal(app[0][b], a_ref), f"approx row {b}"
        assert np.array_equal(y[0][b], O.reconstruct(d_ref, a_ref, *rlohi(w), O.PERIODIC, w.wavelet_id)), f"y row {b}"


@pytest.mark.parametrize("w,N", CASES, ids=lambda v: v.name() if hasattr(v, "name") else str(v))
def test_fma_keep2_is_bit_exact_against_the_fma_restatement(ctxs, w, N):
    """The FMA twin: KEEP = 2 at the row's deepest level, three rows, against reconstruct(decompose(x, fma), fma) of
    tests/restatement_generic.py (one fma(x, f, acc) per tap).  KEEP = 0 / 1 and the two separate kernels are tied to
    it by test_every_variant_gives_the_unfused_bytes."""
    L = len(lohi(w)[0])
    J = vw.max_levels(N, L)
    (det, app, y), fused = run(forced(ctxs, 2, N, L, J, nat.FLAG_FMA), w, 3, N, J, nat.FLAG_FMA, steps=1)
    assert fused == 1
    x = O.fill_uniform(3 * N, 7).reshape(3, N)
    d_ref, a_ref = G.decompose(x, *lohi(w), O.PERIODIC, J, fma=True)
    assert np.array_equal(det[0], d_ref), "details"
    assert np.array_equal(app[0], a_ref), "approx"
    assert np.array_equal(y[0], G.reconstruct(d_ref, a_ref, *rlohi(w), O.PERIODIC, w.wavelet_id, fma=True)), "y"


@pytest.mark.parametrize("N", [512, 1024, 4096])
def test_auto_never_gives_up_a_resident_workgroup(ctxs, N):
    """Auto selection (VW_PAIR_KEEP negative) reports no fewer workgroups per CU than KEEP = 0."""
    auto = vw.Engine(0)
    try:
        auto.set_option("VW_PAIR_KEEP", -1)
        for flags in (0, nat.FLAG_FMA):
            for L in (2, 4, 6, 8):
                k0, n0 = ctxs[0][0][0].roundtrip_variant(N, L, 3, flags)
                k, n = auto.roundtrip_variant(N, L, 3, flags)
                print(f"  N={N} L={L} flags={flags}: auto keeps {k} at {n} per CU; KEEP=0 runs {n0}")
                assert k0 == 0 and n0 >= 1
                assert 0 <= k <= 2 and n >= n0, (L, flags, k, n, n0)
                assert auto.roundtrip_occupancy(N, L, 3, flags) == n
    finally:
        auto.close()
