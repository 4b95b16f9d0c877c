"""vw_icwt_* / InverseCWT on the GPU against the restatement (tests/icwt_restatement.py) on the SAME tables
(vectorwave_amd.cwt.build_inverse_tables -- tests/test_icwt_restatement_cpu.py ties that table form to the reference's
routes).

Shapes, each the smallest that reaches a distinct path of k_icwt / k_icwt_direct:
  N = 128          M = N: pure wrap, no zero region; the tile (64 threads x NV) is larger than the row in fp32
  N = 200          M = 256: the zero region [200, 256)
  N = 1025         M = 2048; fp64: a second tile with one live output
  N = 2049, B = 1  M = 4096; fp64: three tiles
  N = 127, N = 5   the DIRECT form
Scales 0.02 (K = 1), 0.11 .. 0.35 (K = 7 .. 27 for Morlet, with the others every K mod NV for NV = 4 and 8 -- asserted
below), 1 (K = 77), 7 (the un-capped middle) and M / 32 (capped at M taps).  S = 1, 2, 5, a band over planes 2..4 of 6,
B = 1 and 5, padded rows on both sides with NaN padding, host and device memory.

  EXACT  every output's bit pattern equals the restatement's (fp64; fp32 against the same loops at numpy.float32
         with the table, the weights and the divisor rounded once).  A NaN is compared as a NaN, not by its payload.
  FMA    bit for bit against the restatement with one correctly rounded fma per term (inner) and per descriptor
         (outer), and within the derived bound of EXACT (icwt_restatement.fma_bound):
           |fma - exact| <= ( sum_j |weight_j| 2 K_j u sum_k|w_j[k]| max|z|  +  (3 nsc + 2) u A ) / divisor,
           A = sum_j |weight_j| sum_k|w_j[k]| max|z|,  u = 2^-53 or 2^-24
         -- cwt_restatement.fma_bound's per-scale bound carried through the weight, plus the outer sum's roundings
         (nsc sums in either mode and nsc products in EXACT, each of a value at most A) and the division's.
"""
import ctypes
import functools

import numpy as np
import pytest

import icwt_restatement as R
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd.cwt import (CWTConfig, CWTResult, CWTTransform, DOGWavelet, InverseCWT, MorletWavelet, PaulWavelet,
                                RickerWavelet, build_inverse_tables, next_power_of_two)

pytestmark = pytest.mark.gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

WAVELETS = {"morlet": MorletWavelet(), "paul4": PaulWavelet(4), "ricker": RickerWavelet(1.0), "dog2": DOGWavelet(2)}
NP = {"f64": np.float64, "f32": np.float32}
SMALL = [0.02, 0.11, 0.13, 0.16, 0.19, 0.21, 0.24, 0.27, 0.35]   # K = 1, 7, 9, 11, 13, 15, 17, 19, 27 for Morlet


def scales_for(N, S):
    """S ascending scales for rows of N: the K = 1 scale first, then short tables, 1, 7 and one capped at M."""
    M = next_power_of_two(N)
    pool = {1: [1.0], 2: [0.02, M / 32.0], 5: [0.02, 0.16, 1.0, 7.0, M / 32.0], 6: [0.02, 0.13, 0.21, 1.0, 7.0, M / 32.0],
            9: SMALL}[S]
    return sorted(pool)


@functools.lru_cache(maxsize=None)
def _planes(N, B, S, dname, ld=None):
    """Coefficient planes [B, S, ld], fixed per shape."""
    ld = N if ld is None else ld
    a = np.random.default_rng(1000 * N + 10 * B + S).standard_normal((B, S, ld)).astype(NP[dname])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _tables(wname, N, S, start=0, end=None):
    return build_inverse_tables(WAVELETS[wname], scales_for(N, S), N, start, S if end is None else end)


@functools.lru_cache(maxsize=None)
def _expected(wname, N, B, S, dname, fma=False, start=0, end=None, ld=None):
    out = R.reconstruct_rows(_planes(N, B, S, dname, ld), N, _tables(wname, N, S, start, end), NP[dname], fma)
    out.setflags(write=False)
    return out


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _host(a):
    return a.cpu().numpy() if torch is not None and isinstance(a, torch.Tensor) else np.asarray(a)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(got.view(u)[~gn], want.view(u)[~wn])


def _run(engine, planes, t, flags=0, **kw):
    return engine.icwt(planes, t.scales, t.taps, t.form, t.wrap, t.divisor, flags, **kw)


# ---- the table lengths the shapes are chosen for ---------------------------------------------------------------------
def test_the_scales_reach_every_tap_loop_path():
    t = build_inverse_tables(WAVELETS["morlet"], SMALL, 128, 0, len(SMALL))
    K = [d[1] for d in t.scales]
    assert K[0] == 1 and {k % 4 for k in K} == {1, 3} and {k % 8 for k in K} == {1, 3, 5, 7}   # odd: g is cut symmetrically
    # ... Paul's tables never reach 0.0: d in (-M/2, M/2] has an even length, capped at every scale
    assert all(d[1] == 128 for d in build_inverse_tables(WAVELETS["paul4"], SMALL, 128, 0, 9).scales)
    lengths = set()
    for N in (128, 200, 1025, 2049):
        M = next_power_of_two(N)
        t = _tables("morlet", N, 5)
        assert t.form == nat.ICWT_SUM and t.wrap == M
        assert t.scales[0][1] == 1 and t.scales[2][1] == 77 and t.scales[4][1] == M          # K = 1, Morlet at 1, capped
        assert 77 < t.scales[3][1] <= M and (N < 1025 or t.scales[3][1] < M)                 # the un-capped middle
        lengths |= {d[1] for d in t.scales}
    assert max(lengths) == 4096


# ---- EXACT: the SUM form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", [(128, 1), (128, 5), (200, 5), (1025, 5), (2049, 1)])
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_sum_form_bit_equal(engine, N, B, dname):
    for wname, S in (("morlet", 5), ("morlet", 1), ("ricker", 2), ("paul4", 2)) if N < 2049 else (("morlet", 5),):
        t = _tables(wname, N, S)
        got = _run(engine, _dev(_planes(N, B, S, dname)), t)
        assert tuple(got.shape) == (B, N) and got.dtype == (torch.float64 if dname == "f64" else torch.float32)
        assert _same_bits(_host(got), _expected(wname, N, B, S, dname)), f"{wname} N={N} B={B} S={S} {dname}"


@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_every_tap_remainder(engine, dname):
    """Nine short tables of every K mod NV in one call (Morlet), and DOG-2's at the same scales."""
    for wname in ("morlet", "dog2"):
        for N in (128, 200):
            t = _tables(wname, N, 9)
            got = _run(engine, _dev(_planes(N, 5, 9, dname)), t)
            assert _same_bits(_host(got), _expected(wname, N, 5, 9, dname)), f"{wname} N={N} {dname}"


@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_a_band_reads_its_planes_only(engine, dname):
    """Descriptors over planes 2..4 of 6; the other planes hold NaN, which no output may see."""
    for N in (200, 1025):
        t = _tables("morlet", N, 6, 2, 5)
        assert [d[3] for d in t.scales] == [2, 3, 4]
        planes = np.array(_planes(N, 5, 6, dname))
        want = R.reconstruct_rows(planes, N, t, NP[dname])
        planes[:, [0, 1, 5], :] = np.nan
        got = _host(_run(engine, _dev(planes), t))
        assert not np.isnan(got).any() and _same_bits(got, want), f"N={N} {dname}"


@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_padded_rows_and_host_memory(engine, dname):
    """ldc = N + 3 and ldo = N + 5, the padding NaN on both sides: read by no output, and left alone; device, then
    host memory."""
    N, B, S = 200, 5, 5
    ldc, ldo = N + 3, N + 5
    t = _tables("morlet", N, S)
    planes = np.array(_planes(N, B, S, dname, ldc))
    want = R.reconstruct_rows(planes, N, t, NP[dname])
    planes[:, :, N:] = np.nan
    for to in (_dev, np.array):
        out = to(np.full((B, ldo), np.nan, dtype=NP[dname]))
        res = _run(engine, to(planes), t, N=N, out=out)
        assert res is out
        got = _host(out)
        assert _same_bits(got[:, :N], want) and np.isnan(got[:, N:]).all(), (to.__name__, dname)
    res = _run(engine, np.array(_planes(N, B, S, dname)), t)
    assert isinstance(res, np.ndarray) and _same_bits(res, _expected("morlet", N, B, S, dname))


# ---- EXACT: the DIRECT form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 127])
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_direct_form_bit_equal(engine, N, dname):
    for wname, S, B in (("morlet", 5, 5), ("morlet", 1, 1), ("dog2", 2, 5)):
        scales = [0.7] if S == 1 else [0.5, 4.0] if S == 2 else [0.5, 1.0, 2.5, 7.0, 19.0]
        t = build_inverse_tables(WAVELETS[wname], scales, N, 0, S)
        assert t.form == nat.ICWT_DIRECT
        planes = np.array(_planes(N, B, S, dname))
        planes[0, 0, 0] = 0.0
        planes[0, 0, N // 2] = 5e-11          # skipped
        planes[B - 1, S - 1, N - 1] = -5e-11
        want = R.reconstruct_rows(planes, N, t, NP[dname])
        got = _host(_run(engine, _dev(planes), t))
        assert _same_bits(got, want), f"{wname} N={N} S={S} {dname}"
        if B > 1:                             # a NaN is not skipped: its row is NaN throughout, the others are not
            planes[1, S - 1, 1] = np.nan
            got = _host(_run(engine, _dev(planes), t))
            assert _same_bits(got, R.reconstruct_rows(planes, N, t, NP[dname]))
            assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2]]).any()
    # a band over planes 1..2 of 3, padded rows, host memory
    t = build_inverse_tables(WAVELETS["morlet"], [0.5, 2.0, 6.0], N, 1, 3)
    planes = np.array(_planes(N, 5, 3, dname, N + 3))
    want = R.reconstruct_rows(planes, N, t, NP[dname])
    planes[:, :, N:] = np.nan
    planes[:, 0, :] = np.nan
    for to in (_dev, np.array):
        out = to(np.full((5, N + 1), np.nan, dtype=NP[dname]))
        _run(engine, to(planes), t, N=N, out=out)
        got = _host(out)
        assert _same_bits(got[:, :N], want) and np.isnan(got[:, N:]).all(), (to.__name__, N, dname)


def test_the_skipped_coefficient_is_skipped_in_the_element_type(engine):
    """|c| < T(1e-10): a coefficient between float32(1e-10) and 1e-10 is skipped in fp64 and kept in fp32."""
    N = 5
    c32 = np.float32(1e-10)
    assert float(c32) > 1e-10               # float32(1e-10) rounds up
    mid = np.float32(np.nextafter(c32, np.float32(0)))
    assert float(mid) < 1e-10 < float(c32)
    for dname in ("f64", "f32"):
        t = build_inverse_tables(WAVELETS["morlet"], [1.0], N, 0, 1)
        planes = np.zeros((1, 1, N), dtype=NP[dname])
        planes[0, 0, 2] = mid
        got = _host(_run(engine, _dev(planes), t))
        assert _same_bits(got, R.reconstruct_rows(planes, N, t, NP[dname]))
        assert not got.any()                # below the tolerance in either type: every term skipped
        planes[0, 0, 2] = c32
        got = _host(_run(engine, _dev(planes), t))
        assert _same_bits(got, R.reconstruct_rows(planes, N, t, NP[dname]))
        assert got.any()                    # at the fp32 tolerance, above the fp64 one: kept in both


# ---- FMA -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", [(128, 5), (200, 5), (1025, 5), (2049, 1)])
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_fma_bits_and_bound(engine, N, B, dname):
    wname, S = "morlet", 5
    t = _tables(wname, N, S)
    planes = _planes(N, B, S, dname)
    got = _host(_run(engine, _dev(planes), t, nat.FLAG_FMA))
    exact = _expected(wname, N, B, S, dname)
    bound = R.fma_bound(t.scales, t.taps, t.divisor, float(np.max(np.abs(planes))), NP[dname])
    diff = float(np.max(np.abs(got.astype(np.float64) - exact.astype(np.float64))))
    print(f"N={N} {dname}: |fma - exact| = {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound, (diff, bound)
    assert diff > 0.0                        # the FMA build does fuse: some output differs from the separate roundings
    assert _same_bits(got, _expected(wname, N, B, S, dname, True)), f"fma bits N={N} {dname}"


# ---- the C ABI's refusals --------------------------------------------------------------------------------------------
def test_abi_errors(engine):
    """Every refusal of include/vectorwave_amd.h's list, on a live context with real device buffers: no output
    element is written."""
    from test_plan_icwt_cpu import DIRECT, call
    E = vw.errors
    B, S, N = 2, 3, 200
    coef = _dev(_planes(N, B, S, "f64"))
    out = torch.full((B, N), float("nan"), dtype=torch.float64, device="cuda")
    for sfx, cf, ot in (("f64", coef, out), ("f32", coef.float(), out.float())):
        kw = dict(ctx=engine.ctx, coef=ctypes.c_void_p(cf.data_ptr()), out=ctypes.c_void_p(ot.data_ptr()))
        c = functools.partial(call, nat, sfx, **kw)
        assert c() == 0, nat.last_error()
        torch.cuda.synchronize()
        assert not torch.isnan(ot).any()
        ot.fill_(float("nan"))
        assert call(nat, sfx, **dict(kw, ctx=None)) == E.VW_ERR_NULL
        assert call(nat, sfx, **dict(kw, coef=None)) == E.VW_ERR_NULL
        assert call(nat, sfx, **dict(kw, out=None)) == E.VW_ERR_NULL
        assert c(taps=None) == E.VW_ERR_NULL and c(null_scales=True) == E.VW_ERR_NULL
        assert c(B=0) == c(S=0) == c(N=0) == c(scales=()) == E.VW_ERR_EMPTY
        bad = E.VW_ERR_ARG
        assert c(ldc=199) == bad and c(ldo=199) == bad
        assert c(scales=((0, 17, -8, 3, 0.5, 1.0),)) == bad and c(scales=((0, 17, -8, -1, 0.5, 1.0),)) == bad
        assert c(scales=((30, 11, -5, 1, 0.5, 1.0),)) == bad and c(scales=((-1, 17, -8, 0, 0.5, 1.0),)) == bad
        assert c(scales=((0, 0, 0, 0, 0.5, 1.0),)) == bad
        assert c(divisor=0.0) == bad and c(divisor=-1.0) == bad and c(divisor=float("nan")) == bad
        assert c(wrap=199) == bad and c(form=2) == bad and c(flags=nat.FLAG_VALIDATE) == bad
        direct = dict(N=20, ldc=20, ldo=20, form=DIRECT, wrap=0, scales=((0, 39, 0, 0, 0.5, 1.0),))
        assert c(**direct) == 0
        torch.cuda.synchronize()
        ot.fill_(float("nan"))
        assert c(**dict(direct, flags=nat.FLAG_FMA)) == bad
        assert c(**dict(direct, scales=((0, 38, 0, 0, 0.5, 1.0),))) == bad
        table = np.zeros(40000)
        tp = table.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert c(scales=((0, 17, -8, 0, 0.5, 1.0), (0, 16385, -8192, 1, 0.5, 1.0)), table=tp, ntaps=40000) == E.VW_ERR_UNSUPPORTED
        assert "scale 1" in nat.last_error()
        torch.cuda.synchronize()
        assert torch.isnan(ot).all()
    with pytest.raises(vw.InvalidArgumentException, match="VW_FLAG_FMA"):
        t = build_inverse_tables(WAVELETS["morlet"], [1.0], 20, 0, 1)
        _run(engine, _dev(_planes(20, 1, 1, "f64")), t, nat.FLAG_FMA)
    with pytest.raises(NotImplementedError, match="scale 0"):
        engine.icwt(coef, [(0, 16385, -8192, 0, 1.0, 1.0)], np.zeros(16385), nat.ICWT_SUM, 256, 1.0)


# ---- graphs and the table slots --------------------------------------------------------------------------------------
def test_a_call_with_resident_tables_replays_from_a_graph(engine):
    """Once a call has put its tables on the device the same call can be recorded, with a forward CWT call in between
    (the two keep their images in slots of their own); a call with new tables cannot."""
    from vectorwave_amd.cwt import build_tables
    N, B, S = 200, 5, 5
    t, other = _tables("morlet", N, S), _tables("ricker", N, 2)
    want = _expected("morlet", N, B, S, "f64")
    fwd = build_tables(WAVELETS["ricker"], CWTConfig.defaultConfig(), [1.0, 3.0], N)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        planes = _dev(_planes(N, B, S, "f64"))
        x = _dev(_planes(N, B, 1, "f64")[:, 0, :])
        forward = lambda: engine.cwt(x, fwd.scales, fwd.taps_re, fwd.taps_im, fwd.ext, fwd.wrap, 0)   # noqa: E731
        step = lambda: _run(engine, planes, t)                                                         # noqa: E731
        step()
        forward()
        both = engine.capture(lambda: (forward(), step()))       # neither call uploads: both images are resident
        out = both.result[1]
        out.fill_(float("nan"))
        both.launch(2)
        torch.cuda.synchronize()
        assert _same_bits(_host(out), want), "graph replay"
        both.close()
        planes2 = _dev(_planes(N, B, 2, "f64"))
        with pytest.raises(vw.InvalidStateException, match="tables"):
            engine.capture(lambda: _run(engine, planes2, other))
        torch.cuda.synchronize()
    engine.bind_torch_stream()


def test_timing_family(engine):
    N, B, S = 200, 5, 5
    t = _tables("morlet", N, S)
    planes = _dev(_planes(N, B, S, "f64"))
    lib, ms, n = engine.lib, ctypes.c_double(), ctypes.c_int64()
    assert lib.vw_ctx_enable_timing(engine.ctx, 1) == 0 and lib.vw_ctx_reset_timing(engine.ctx) == 0
    try:
        _run(engine, planes, t)
        _run(engine, planes, t)
        torch.cuda.synchronize()
        assert lib.vw_ctx_kernel_time(engine.ctx, b"icwt", ctypes.byref(ms), ctypes.byref(n)) == 0
        assert n.value == 2 and ms.value > 0.0
        assert lib.vw_ctx_kernel_time(engine.ctx, b"cwt", ctypes.byref(ms), ctypes.byref(n)) == 0 and n.value == 0
    finally:
        lib.vw_ctx_enable_timing(engine.ctx, 0)


# ---- facade ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_reconstruct_of_analyze(engine, dname):
    """InverseCWT(...).reconstruct(CWTTransform(...).analyze(x, scales)) on a device tensor: the restatement fed the
    same planes, both routes, one row and a batch; and the bands."""
    scales = [1.0, 2.0, 4.0, 8.0, 16.0]
    for wname, N, B in (("morlet", 200, 3), ("ricker", 1025, 2), ("morlet", 100, 3)):
        w = WAVELETS[wname]
        x = _dev(np.random.default_rng(N).standard_normal((B, N)).astype(NP[dname]))
        res = CWTTransform(w, CWTConfig.defaultConfig()).analyze(x, scales)
        inv = InverseCWT(w)
        got = inv.reconstruct(res)
        planes = _host(res.getCoefficients())
        t = build_inverse_tables(w, scales, N, 0, len(scales))
        assert t.form == (nat.ICWT_SUM if N >= 128 else nat.ICWT_DIRECT)
        assert isinstance(got, torch.Tensor) and tuple(got.shape) == (B, N)
        assert _same_bits(_host(got), R.reconstruct_rows(planes, N, t, NP[dname])), (wname, N, dname)
        one = inv.reconstruct(CWTResult(res.getReal()[1], None, scales, w))
        assert tuple(one.shape) == (N,) and torch.equal(one, got[1])
        band = inv.reconstructBand(res, 2.0, 8.0)                 # planes 1..3
        tb = build_inverse_tables(w, scales, N, 1, 4)
        assert _same_bits(_host(band), R.reconstruct_rows(planes, N, tb, NP[dname])), (wname, N, dname, "band")
        cf = w.centerFrequency()
        fband = inv.reconstructFrequencyBand(res, 100.0, cf * 100.0 / 12.0, cf * 100.0 / 3.0)   # scales in [3, 12]
        tf = build_inverse_tables(w, scales, N, 2, 4)
        assert _same_bits(_host(fband), R.reconstruct_rows(planes, N, tf, NP[dname])), (wname, N, dname, "frequency band")
        zero = inv.reconstructBand(res, 2.5, 3.0)
        assert isinstance(zero, torch.Tensor) and tuple(zero.shape) == (B, N) and not zero.any()
        host = inv.reconstruct(CWTResult(planes, None, scales, w))   # numpy planes: host memory, the same bits
        assert isinstance(host, np.ndarray) and _same_bits(host, _host(got))
        fused = InverseCWT(w, fma=True).reconstruct(res)          # N < 128: the flag is dropped
        if N < 128:
            assert torch.equal(fused, got)
        else:
            assert _same_bits(_host(fused), R.reconstruct_rows(planes, N, t, NP[dname], True))
