"""VW_PAIR_FUSE: a captured forward followed by the inverse of its coefficients is recorded as ONE k_roundtrip launch.

The round-trip kernel (vw_pair.hip) runs the persistent forward's loop body and then the PLAIN inverse's schedule on
the same row, keeping a_J and d_J in registers and reading d_{J-1} .. d_1 back right after storing them.  Per
output the operation sequence is that of the two separate kernels, so with the switch on and off -- two contexts,
the way tests/test_gpu_inverse_waves.py switches VW_INV_WAVES -- details, approx and y are the same BYTES, EXACT is
bit-exact against the restatement, FMA bit-exact against the restatement's FMA form (tests/restatement_generic.py
``fma=True``), and vw_graph_stats says what the capture recorded: K fused pairs, or none.

Shapes are the smallest at which each mechanism can go wrong: N = 512 (one wave per workgroup; at deep levels the
right halo spans more than the first slab, so it is copied after a barrier), N = 1024, N = 4096 (8 waves); J = 1 (no
reload at all), J = 2 and the deepest level the row allows; B = 1, 3 and, at N = 512, twice the resident grid plus 5
(the persistent loop, the next-row prefetch and the buffer swap run more than one row per workgroup).
Everything the kernel does not cover falls through to the two kernels, bytes unchanged.
"""
from ctypes import c_uint64, c_void_p

import numpy as np
import pytest

from oracle import oracle as O
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import Daubechies, Haar, Symlet

import restatement_generic as G

pytestmark = pytest.mark.gpu

K = 3
# haar, db2, db3, db4: 2, 4, 6 and 8 taps (sym3: the catalogue's six-tap Daubechies-3)
WAVELETS = [Haar.INSTANCE, Daubechies.DB2, Symlet.SYM3, Daubechies.DB4]


def lohi(w):
    return w.lowPassDecomposition(), w.highPassDecomposition()


def rlohi(w):
    return w.lowPassReconstruction(), w.highPassReconstruction()


@pytest.fixture(scope="module")
def pair(engine):
    """(context with VW_PAIR_FUSE=1, context with VW_PAIR_FUSE=0), each on a stream of its own."""
    import torch
    on, off = vw.Engine(0), vw.Engine(0)
    on.set_option("VW_PAIR_FUSE", 1)
    off.set_option("VW_PAIR_FUSE", 0)
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    yield (on, streams[0]), (off, streams[1])
    torch.cuda.synchronize()
    on.close()
    off.close()


class Case:
    """One forward -> inverse pair; the keyword arguments are the fall-through variants."""

    def __init__(self, w, B, N, J, flags, boundary=O.PERIODIC, f32=False, mask=0xFFFFFFFF, between=False,
                 other_details=False, alias_y=False, timing=False, steps=K, seed=7):
        self.w, self.B, self.N, self.J, self.flags, self.boundary = w, B, N, J, flags, boundary
        self.f32, self.mask, self.between, self.other_details = f32, mask, between, other_details
        self.alias_y, self.timing, self.steps, self.seed = alias_y, timing, steps, seed


def run(eng_stream, c):
    """Capture c.steps forward -> inverse pairs on the context, replay the graph once (and once more), return
    (details, approx, y) of every step as numpy arrays plus vw_graph_stats' (kernel nodes, fused pairs)."""
    import torch
    eng, stream = eng_stream
    lib, ctx = eng.lib, eng.ctx
    dt = torch.float32 if c.f32 else torch.float64
    fwd = lib.vw_modwt_forward_f32 if c.f32 else lib.vw_modwt_forward_f64
    inv = lib.vw_modwt_inverse_f32 if c.f32 else lib.vw_modwt_inverse_f64
    lo, hi = (nat.taps_array(t) for t in lohi(c.w))
    rlo, rhi = (nat.taps_array(t) for t in rlohi(c.w))
    L = len(lohi(c.w)[0])
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    S, B, N, J = c.steps, c.B, c.N, c.J
    with torch.cuda.stream(stream):
        eng.bind_torch_stream()
        x = torch.empty((S, B, N), dtype=dt, device="cuda")
        det = torch.empty((S, J, B, N), dtype=dt, device="cuda")
        app = torch.empty((S, B, N), dtype=dt, device="cuda")
        y = x if c.alias_y else torch.empty((S, B, N), dtype=dt, device="cuda")
        det2 = torch.empty((S, J, B, N), dtype=dt, device="cuda") if c.other_details else None
        junk = torch.empty((64,), dtype=torch.float64, device="cuda")

        def step(k):
            assert fwd(ctx, P(x[k]), B, N, N, lo, hi, L, c.w.wavelet_id, c.boundary, J, c.flags, P(det[k]),
                       P(app[k])) == 0, nat.last_error()
            if c.between:  # another engine call recorded between the two
                assert lib.vw_fill_uniform_f64(ctx, P(junk), 64, c_uint64(1), 0) == 0
            src = det2 if c.other_details else det
            assert inv(ctx, P(src[k]), P(app[k]), B, N, rlo, rhi, L, c.w.wavelet_id, c.boundary, J, c.mask, 0, c.flags,
                       P(y[k])) == 0, nat.last_error()

        def fill():
            eng.fill_uniform(x, c.seed)

        fill()
        for k in range(S):  # outside any capture: LDS limits, occupancy, workspaces
            step(k)
        torch.cuda.synchronize()
        if c.other_details:
            det2.copy_(det)
        if c.timing:
            eng.enable_timing(True)
        try:
            g = eng.capture(lambda: [step(k) for k in range(S)])
        finally:
            if c.timing:
                eng.enable_timing(False)
                eng.reset_timing()
        stats = g.stats()
        out = []
        for _ in range(2):  # a replay, then a second one: the same bytes
            fill()
            for t in (det, app) + (() if c.alias_y else (y,)):
                t.fill_(float("nan"))
            g.launch(1)
            torch.cuda.synchronize()
            out.append(tuple(t.cpu().numpy().copy() for t in (det, app, y)))
        g.close()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b, equal_nan=True), "a second replay of the graph gives other bytes"
    assert not any(np.isnan(a).any() for a in out[0]), "an output was not written"
    return out[0], stats


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def levels_of(N, L):
    return sorted({1, 2, vw.max_levels(N, L)})


@pytest.mark.parametrize("N", [512, 1024, 4096])
@pytest.mark.parametrize("w", WAVELETS, ids=lambda w: w.name())
def test_fused_and_unfused_captures_give_the_same_bytes(pair, w, N):
    on, off = pair
    L = len(lohi(w)[0])
    for J in levels_of(N, L):
        for flags in (0, nat.FLAG_FMA):
            for B in (1, 3):
                c = Case(w, B, N, J, flags)
                got, (kernels, fused) = run(on, c)
                ref, (kernels0, fused0) = run(off, c)
                print(f"  {w.name()} N={N} J={J} flags={flags} B={B}: kernel nodes {kernels} / {kernels0}, "
                      f"fused {fused} / {fused0}")
                assert fused == K and kernels == K, (J, flags, B, kernels, fused)
                assert fused0 == 0 and kernels0 == 2 * K, (J, flags, B, kernels0, fused0)
                assert same_bytes(got, ref), f"J={J} flags={flags} B={B}: fused differs from unfused"


@pytest.mark.parametrize("w", WAVELETS, ids=lambda w: w.name())
def test_exact_is_bit_exact_against_the_restatement(pair, w):
    """One case per wavelet: N = 1024 at its deepest level, three rows, EXACT."""
    on, _ = pair
    N = 1024
    J = vw.max_levels(N, len(lohi(w)[0]))
    (det, app, y), (_, fused) = run(on, Case(w, 3, N, J, 0, steps=1))
    assert fused == 1
    x = O.fill_uniform(3 * N, 7).reshape(3, N)
    for b in range(3):
        d_ref, a_ref = O.decompose(x[b], *lohi(w), O.PERIODIC, J, core=False)
        assert np.array_equal(det[0][:, b, :], d_ref), f"details row {b}"
        assert np.array_equal(app[0][b], a_ref), f"approx row {b}"
        assert np.array_equal(y[0][b], O.reconstruct(d_ref, a_ref, *rlohi(w), O.PERIODIC, w.wavelet_id)), f"y row {b}"


@pytest.mark.parametrize("w", WAVELETS, ids=lambda w: w.name())
def test_fma_is_bit_exact_against_the_fma_restatement(pair, w):
    """The FMA twin, at every N of this file: the captured round trip equals reconstruct(decompose(x, fma), fma) --
    one fma(x, f, acc) per tap -- at the row's deepest level, three rows.  Every other FMA variant here is tied to
    this one by the "same bytes" tests."""
    on, _ = pair
    for N in (512, 1024, 4096):
        J = vw.max_levels(N, len(lohi(w)[0]))
        (det, app, y), (_, fused) = run(on, Case(w, 3, N, J, nat.FLAG_FMA, steps=1))
        assert fused == 1
        x = O.fill_uniform(3 * N, 7).reshape(3, N)
        d_ref, a_ref = G.decompose(x, *lohi(w), O.PERIODIC, J, fma=True)
        y_ref = G.reconstruct(d_ref, a_ref, *rlohi(w), O.PERIODIC, w.wavelet_id, fma=True)
        assert np.array_equal(det[0], d_ref), f"N={N} details"
        assert np.array_equal(app[0], a_ref), f"N={N} approx"
        assert np.array_equal(y[0], y_ref), f"N={N} y"


@pytest.mark.parametrize("J,flags", [(2, nat.FLAG_FMA), (3, 0)], ids=["J2-fma", "J3-exact"])
def test_more_rows_than_resident_workgroups(pair, J, flags):
    """N = 512, B = twice the resident grid + 5: every workgroup walks two or three rows.  J even and odd: the level
    buffer the next row lands in alternates with the parity of J."""
    import torch
    on, off = pair
    w = Daubechies.DB4
    per_cu = on[0].roundtrip_occupancy(512, 8, J, flags)
    assert per_cu >= 1
    B = 2 * per_cu * torch.cuda.get_device_properties(0).multi_processor_count + 5
    c = Case(w, B, 512, J, flags, steps=1)
    got, (_, fused) = run(on, c)
    ref, (_, fused0) = run(off, c)
    print(f"  {per_cu} workgroups per CU, B = {B}")
    assert fused == 1 and fused0 == 0
    assert same_bytes(got, ref)


@pytest.mark.parametrize("N", [512, 1024, 4096])
def test_uncaptured_roundtrip_call(pair, engine, N):
    """vw_modwt_roundtrip_f64 outside a capture: the bytes of forward followed by inverse."""
    import torch
    on, off = pair
    for w in WAVELETS:
        L = len(lohi(w)[0])
        for J in levels_of(N, L):
            for flags in (0, nat.FLAG_FMA):
                for B in (1, 3):
                    x = torch.empty((B, N), dtype=torch.float64, device="cuda")
                    engine.fill_uniform(x, 11)
                    torch.cuda.synchronize()
                    with torch.cuda.stream(on[1]):
                        det, app, y = on[0].roundtrip(x, *lohi(w), *rlohi(w), w.wavelet_id, O.PERIODIC, J, flags)
                    with torch.cuda.stream(off[1]):
                        det0, app0 = off[0].forward(x, *lohi(w), w.wavelet_id, O.PERIODIC, J, flags)
                        y0 = off[0].inverse(det0, app0, *rlohi(w), w.wavelet_id, O.PERIODIC, J, flags)
                    torch.cuda.synchronize()
                    assert torch.equal(det, det0) and torch.equal(app, app0) and torch.equal(y, y0), \
                        (w.name(), J, flags, B)


FALL_THROUGH = {
    "call-between": dict(between=True),
    "other-details-buffer": dict(other_details=True),
    "one-level-masked": dict(mask=0xFFFFFFFF & ~2),
    "ref-nonfinite": dict(flags=nat.FLAG_FMA | nat.FLAG_REF_NONFINITE),
    "timing-enabled": dict(timing=True),
    "y-aliases-x": dict(alias_y=True),
    "symmetric": dict(boundary=O.SYMMETRIC),
    "fp32": dict(f32=True),
    "sym8": dict(w=Symlet.SYM8),
    "N4100": dict(N=4100),
}


@pytest.mark.parametrize("name", list(FALL_THROUGH))
def test_what_the_kernel_does_not_cover_stays_two_kernels(pair, name):
    on, off = pair
    kw = dict(w=Daubechies.DB4, B=3, N=512, J=3, flags=nat.FLAG_FMA)
    kw.update(FALL_THROUGH[name])
    c = Case(**kw)
    got, (_, fused) = run(on, c)
    ref, (_, fused0) = run(off, c)
    assert fused == 0 and fused0 == 0, (fused, fused0)
    assert same_bytes(got, ref)
