"""Biorthogonal banks (two filter lengths) on the GPU: the vw_modwt_*_bi_* entry points and the facades over them.

Reference: tests/restatement_bi.py (pinned on the CPU by tests/test_restatement_bi_cpu.py).  Wavelets chosen for
their length patterns (analysis pair): bior1.1 (2,2), bior1.3 (6,2), bior2.2 (5,3), bior4.4 (9,7), bior3.9 (20,4),
bior6.8 (17,16), rbio1.5 (2,10), rbio4.4 (7,9); the synthesis pair is the swap.

Bars: EXACT bit-exact against the restatement.  FMA bit-exact against the restatement's FMA form (``fma=True``: each
filter's own ``fma(x, f, acc)`` chain, the pairwise inverses ``acc + fma(lo, a, round(hi * d))``) and, as before, fp64 within 1e-12 * max(1, max|restatement|): the suite's
1e-12 scaled by magnitude, because these banks are not normalised (the bound itself is at most (Llo + Lhi) * 2^-53
of a level's largest magnitude per level, <= 2e-14 relative for J <= 4, L <= 20).  FMA fp32 within
1e-5 * J * max(1, max|restatement|): the suite's fp32 bar (tests/test_gpu_f32_parity.py) scaled the same way.
Signals are O.java_random_signal, B = 3, device tensors, no validation flags unless stated.

A second anchor that needs no new restatement: where the reference's loops visit each filter on its own (forward
P / S / Z, PERIODIC inverse) the two-length call equals the EXISTING equal-length call on zero-extended filters bit
for bit, and with Llo == Lhi the _bi_ entry points are the existing ones.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
import vectorwave_amd as vw
from vectorwave_amd import _native as nat
from vectorwave_amd.errors import ErrorCode, InvalidArgumentException
from vectorwave_amd.wavelets import WID_OTHER, Daubechies, get_wavelet

import restatement_bi as R

pytestmark = pytest.mark.gpu

NAMES = ["bior1.1", "bior1.3", "bior2.2", "bior4.4", "bior3.9", "bior6.8", "rbio1.5", "rbio4.4"]
BOUNDARIES = [O.PERIODIC, O.SYMMETRIC, O.ZERO_PADDING]
BIDS = ["P", "S", "Z"]
DTYPES = {"f64": (np.float64, torch.float64), "f32": (np.float32, torch.float32)}


def analysis(w):
    return w.lowPassDecomposition(), w.highPassDecomposition()


def synthesis(w):
    return w.lowPassReconstruction(), w.highPassReconstruction()


def pairwise_throws(w):
    """The pairwise inverses index high[l] for l < Llo: a shorter synthesis high-pass is the reference's
    ArrayIndexOutOfBoundsException, VW_ERR_UNSUPPORTED here."""
    lo, hi = synthesis(w)
    return len(hi) < len(lo)


def level_cap(w, n, want=4):
    L = max(len(w.lowPassDecomposition()), len(w.highPassDecomposition()))
    return min(want, O.max_levels(n, L))


@functools.lru_cache(maxsize=None)
def signals(B, n, seed=7):
    x = np.stack([O.java_random_signal(n, seed + b) for b in range(B)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def forward_ref(name, boundary, B, n, J, dt):
    det, app = R.decompose(signals(B, n), *analysis(get_wavelet(name)), boundary, J, dtype=DTYPES[dt][0])
    det.setflags(write=False)
    app.setflags(write=False)
    return det, app


@functools.lru_cache(maxsize=None)
def forward_ref_fma(name, boundary, B, n, J, dt):
    det, app = R.decompose(signals(B, n), *analysis(get_wavelet(name)), boundary, J, dtype=DTYPES[dt][0], fma=True)
    det.setflags(write=False)
    app.setflags(write=False)
    return det, app


def dev(a, dt="f64"):
    return torch.from_numpy(np.array(a, dtype=DTYPES[dt][0])).cuda()


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def exact(a, b, what=""):
    a, b = host(a), host(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if not np.array_equal(a, b, equal_nan=True):
        bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        i = np.unravel_index(np.argmax(bad), a.shape)
        raise AssertionError(f"{what}: not bit-exact at {i}: {a[i]!r} vs {b[i]!r} ({int(bad.sum())} differ)")


def close(a, b, tol, what=""):
    a, b = host(a), host(b)
    err = float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))
    print(f"{what}: FMA max |diff| = {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (what, err, tol)


def fma_tol(dt, J, *refs):
    mag = max(1.0, max(float(np.max(np.abs(r))) for r in refs))
    return 1e-12 * mag if dt == "f64" else 1e-5 * J * mag


# ---- 1. transforms: forward and inverse, f64 / f32, every N mod 4 ------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_transforms(engine, name, boundary):
    """Against the restatement, under the default (VW_BI = 3: the two-length kernels for the compile-time pairs, the
    padded route for the rest) and under VW_BI = 7 (the runtime-L two-length bodies for every other pair too)."""
    for opts in (dict(), dict(VW_BI=7)):
        with engine.options(**opts):
            _transforms(engine, name, boundary)


def _transforms(engine, name, boundary):
    w, B = get_wavelet(name), 3
    for n in (64, 67, 258, 1000, 4096):
        J = level_cap(w, n)
        assert J >= 1
        full = (1 << J) - 1
        for dt in DTYPES:
            what = f"{name} N={n} J={J} {dt}"
            d_ref, a_ref = forward_ref(name, boundary, B, n, J, dt)
            x = dev(signals(B, n), dt)
            det, app = engine.forward(x, *analysis(w), WID_OTHER, boundary, J, 0)
            exact(det, d_ref, what + " details")
            exact(app, a_ref, what + " approx")
            det_f, app_f = engine.forward(x, *analysis(w), WID_OTHER, boundary, J, nat.FLAG_FMA)
            tol = fma_tol(dt, J, d_ref, a_ref)
            d_fma, a_fma = forward_ref_fma(name, boundary, B, n, J, dt)
            exact(det_f, d_fma, what + " FMA details")
            exact(app_f, a_fma, what + " FMA approx")
            close(det_f, d_ref, tol, what + " details")
            close(app_f, a_ref, tol, what + " approx")
            # inverse of the restatement's coefficients: plain, reconstructFromLevel / reconstructLevels masks,
            # zero approximation
            d_in, a_in = dev(d_ref, dt), dev(a_ref, dt)
            for mask, az in ((full, False), (0b110 & full, False), (0b001, True)):
                args = (d_in if mask else None, None if az else a_in, *synthesis(w), WID_OTHER, boundary, J)
                kw = dict(detail_mask=mask, approx_zero=az, shape=(B, n))
                if boundary == O.ZERO_PADDING and pairwise_throws(w):
                    with pytest.raises(NotImplementedError, match="high-pass"):
                        engine.inverse(*args, 0, **kw)
                    continue
                y_ref = R.reconstruct(d_ref, a_ref, *synthesis(w), boundary, WID_OTHER, mask, az, dtype=DTYPES[dt][0])
                exact(engine.inverse(*args, 0, **kw), y_ref, f"{what} inverse mask={mask:b} az={az}")
                y_fma = R.reconstruct(d_ref, a_ref, *synthesis(w), boundary, WID_OTHER, mask, az, dtype=DTYPES[dt][0],
                                      fma=True)
                exact(engine.inverse(*args, nat.FLAG_FMA, **kw), y_fma, f"{what} FMA inverse mask={mask:b} az={az}")
                close(engine.inverse(*args, nat.FLAG_FMA, **kw), y_ref, fma_tol(dt, J, y_ref, d_ref, a_ref),
                      f"{what} inverse mask={mask:b} az={az}")
    torch.cuda.synchronize()


# ---- 2. the existing kernels as a second anchor -------------------------------------------------------------------
def pad(f, L):
    return list(f) + [0.0] * (L - len(f))


@pytest.mark.parametrize("name", [n for n in NAMES if n != "bior1.1"])
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_equals_the_equal_length_call_on_zero_extended_filters(engine, name, boundary):
    w, B = get_wavelet(name), 3
    lo, hi = analysis(w)
    L = max(len(lo), len(hi))
    for n in (258, 4096):
        J = level_cap(w, n)
        for dt in DTYPES:
            x = dev(signals(B, n), dt)
            for flags in (0, nat.FLAG_FMA):
                det, app = engine.forward(x, lo, hi, WID_OTHER, boundary, J, flags)
                det_p, app_p = engine.forward(x, pad(lo, L), pad(hi, L), WID_OTHER, boundary, J, flags)
                assert torch.equal(det, det_p) and torch.equal(app, app_p), (n, dt, flags)
                if boundary == O.PERIODIC:
                    rl, rh = synthesis(w)
                    y = engine.inverse(det, app, rl, rh, WID_OTHER, boundary, J, flags)
                    y_p = engine.inverse(det, app, pad(rl, L), pad(rh, L), WID_OTHER, boundary, J, flags)
                    assert torch.equal(y, y_p), (n, dt, flags)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["bior2.2", "bior4.4", "bior6.8", "rbio4.4"])   # longer filter of 5 / 9 / 17 / 9 taps
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_listed_tap_count_changes_no_bit(engine, name, boundary):
    """By default an unlisted longer length runs one zero tap further, on the tap-unrolled kernels of the next listed
    count (VW_BI_LISTED); with the switch off it runs the runtime-L kernels.  Same bits, EXACT and FMA."""
    w, B = get_wavelet(name), 3
    for n, J in ((258, 3), (4096, 4), (32768, 5)):
        Bn = 2 if n == 32768 else B
        for dt in DTYPES:
            x = dev(signals(Bn, n), dt)
            for flags in (0, nat.FLAG_FMA):
                outs = []
                for listed in (1, 0):
                    with engine.options(VW_BI=0, VW_BI_LISTED=listed):   # the padded route's two tap counts
                        det, app = engine.forward(x, *analysis(w), WID_OTHER, boundary, J, flags)
                        y = None
                        if not (boundary == O.ZERO_PADDING and pairwise_throws(w)):
                            y = engine.inverse(det, app, *synthesis(w), WID_OTHER, boundary, J, flags)
                        outs.append((det, app, y))
                for t1, t0 in zip(*outs):
                    assert (t1 is None and t0 is None) or torch.equal(t1, t0), (n, dt, flags)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", [n for n in NAMES if n != "bior1.1"])
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_two_length_route_equals_padded_route(engine, name, boundary):
    """VW_BI = 7 (the two-length forms of the fused forward and of the fused sequential inverses, each filter at its
    own tap count: the compile-time pairs and, bit 2, the runtime-L bodies for every other pair) equals VW_BI = 0 (zero-extended filters on the equal-length kernels) bit for bit,
    EXACT and FMA, with both sequential kernels (one and two LDS buffers) and the reconstruct masks."""
    w, B = get_wavelet(name), 3
    for n in (64, 67, 258, 1000, 4096):
        J = level_cap(w, n)
        full = (1 << J) - 1
        for dt in DTYPES:
            d_ref, a_ref = forward_ref(name, boundary, B, n, J, dt)
            d_in, a_in = dev(d_ref, dt), dev(a_ref, dt)
            x = dev(signals(B, n), dt)
            for flags in (0, nat.FLAG_FMA):
                for buf in (1, 2):
                    outs = []
                    for bi in (7, 0):
                        with engine.options(VW_BI=bi, VW_INV_BUF=buf):
                            got = list(engine.forward(x, *analysis(w), WID_OTHER, boundary, J, flags))
                            if not (boundary == O.ZERO_PADDING and pairwise_throws(w)):
                                for mask, az in ((full, False), (0b110 & full, False), (0b001, True)):
                                    got.append(engine.inverse(d_in if mask else None, None if az else a_in, *synthesis(w),
                                                              WID_OTHER, boundary, J, flags, detail_mask=mask,
                                                              approx_zero=az, shape=(B, n)))
                            outs.append(got)
                    for t1, t0 in zip(*outs):
                        assert torch.equal(t1, t0), (n, dt, flags, buf)
    torch.cuda.synchronize()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("w", [get_wavelet("bior1.1"), Daubechies.DB4], ids=["bior1.1", "db4"])
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_equal_lengths_are_the_existing_entry_points(engine, w, boundary):
    lib, B, n, J = nat.load(), 3, 1000, 3
    lo, hi = analysis(w)
    rl, rh = synthesis(w)
    L = len(lo)
    for dt, sfx in (("f64", "f64"), ("f32", "f32")):
        x = dev(signals(B, n), dt)
        engine.bind_torch_stream()
        out = [torch.empty((J, B, n), dtype=x.dtype, device="cuda") for _ in range(2)]
        app = [torch.empty((B, n), dtype=x.dtype, device="cuda") for _ in range(2)]
        y = [torch.empty((B, n), dtype=x.dtype, device="cuda") for _ in range(2)]
        st = getattr(lib, "vw_modwt_forward_" + sfx)(engine.ctx, _p(x), B, n, n, nat.taps_array(lo), nat.taps_array(hi),
                                                    L, w.wavelet_id, boundary, J, 0, _p(out[0]), _p(app[0]))
        assert st == 0, nat.last_error()
        st = getattr(lib, "vw_modwt_forward_bi_" + sfx)(engine.ctx, _p(x), B, n, n, nat.taps_array(lo), L,
                                                       nat.taps_array(hi), L, w.wavelet_id, boundary, J, 0,
                                                       _p(out[1]), _p(app[1]))
        assert st == 0, nat.last_error()
        st = getattr(lib, "vw_modwt_inverse_" + sfx)(engine.ctx, _p(out[0]), _p(app[0]), B, n, nat.taps_array(rl),
                                                    nat.taps_array(rh), L, w.wavelet_id, boundary, J, 0xFFFFFFFF, 0, 0,
                                                    _p(y[0]))
        assert st == 0, nat.last_error()
        st = getattr(lib, "vw_modwt_inverse_bi_" + sfx)(engine.ctx, _p(out[0]), _p(app[0]), B, n, nat.taps_array(rl), L,
                                                       nat.taps_array(rh), L, w.wavelet_id, boundary, J, 0xFFFFFFFF, 0,
                                                       0, _p(y[1]))
        assert st == 0, nat.last_error()
        torch.cuda.synchronize()
        assert torch.equal(out[0], out[1]) and torch.equal(app[0], app[1]) and torch.equal(y[0], y[1]), dt
    # single level, fp64
    x = dev(signals(B, n))
    a = [torch.empty((B, n), dtype=x.dtype, device="cuda") for _ in range(2)]
    d = [torch.empty((B, n), dtype=x.dtype, device="cuda") for _ in range(2)]
    y = [torch.empty((B, n), dtype=x.dtype, device="cuda") for _ in range(2)]
    assert lib.vw_modwt1_forward_f64(engine.ctx, _p(x), B, n, n, nat.taps_array(lo), nat.taps_array(hi), L, boundary, 0,
                                     _p(a[0]), _p(d[0])) == 0
    assert lib.vw_modwt1_forward_bi_f64(engine.ctx, _p(x), B, n, n, nat.taps_array(lo), L, nat.taps_array(hi), L,
                                        boundary, 0, _p(a[1]), _p(d[1])) == 0
    assert lib.vw_modwt1_inverse_f64(engine.ctx, _p(a[0]), _p(d[0]), B, n, nat.taps_array(rl), nat.taps_array(rh), L,
                                     boundary, 0, _p(y[0])) == 0
    assert lib.vw_modwt1_inverse_bi_f64(engine.ctx, _p(a[0]), _p(d[0]), B, n, nat.taps_array(rl), L, nat.taps_array(rh),
                                        L, boundary, 0, _p(y[1])) == 0
    torch.cuda.synchronize()
    assert torch.equal(a[0], a[1]) and torch.equal(d[0], d[1]) and torch.equal(y[0], y[1])


def test_filter_length_limits(engine):
    lib, B, n = nat.load(), 2, 256
    x = dev(signals(B, n))
    det = torch.empty((1, B, n), dtype=torch.float64, device="cuda")
    app = torch.empty((B, n), dtype=torch.float64, device="cuda")
    taps = nat.taps_array([0.1] * 65)
    for llo, lhi in ((4, 65), (4, 0), (65, 4), (0, 4)):
        st = lib.vw_modwt_forward_bi_f64(engine.ctx, _p(x), B, n, n, taps, llo, taps, lhi, WID_OTHER, O.PERIODIC, 1, 0,
                                         _p(det), _p(app))
        assert st == vw.errors.VW_ERR_ARG, (llo, lhi, st)
        st = lib.vw_modwt_inverse_bi_f64(engine.ctx, _p(det), _p(app), B, n, taps, llo, taps, lhi, WID_OTHER,
                                         O.PERIODIC, 1, 1, 0, 0, _p(x))
        assert st == vw.errors.VW_ERR_ARG, (llo, lhi, st)


# ---- 3. long-signal path ------------------------------------------------------------------------------------------
def _long_case(engine, name, boundary, B, n, J):
    w = get_wavelet(name)
    d_ref, a_ref = forward_ref(name, boundary, B, n, J, "f64")
    x = dev(signals(B, n))
    det, app = engine.forward(x, *analysis(w), WID_OTHER, boundary, J, 0)
    exact(det, d_ref, "details")
    exact(app, a_ref, "approx")
    det_f, app_f = engine.forward(x, *analysis(w), WID_OTHER, boundary, J, nat.FLAG_FMA)
    d_fma, a_fma = forward_ref_fma(name, boundary, B, n, J, "f64")
    exact(det_f, d_fma, "FMA details")
    exact(app_f, a_fma, "FMA approx")
    close(det_f, d_ref, fma_tol("f64", J, d_ref, a_ref), "details")
    close(app_f, a_ref, fma_tol("f64", J, d_ref, a_ref), "approx")
    y_ref = R.reconstruct(d_ref, a_ref, *synthesis(w), boundary)   # bior synthesis pairs: Lhi >= Llo (ZERO truncates)
    y = engine.inverse(det, app, *synthesis(w), WID_OTHER, boundary, J, 0)
    exact(y, y_ref, "inverse")
    y_f = engine.inverse(det, app, *synthesis(w), WID_OTHER, boundary, J, nat.FLAG_FMA)
    exact(y_f, R.reconstruct(d_ref, a_ref, *synthesis(w), boundary, fma=True), "FMA inverse")
    close(y_f, y_ref, fma_tol("f64", J, y_ref, d_ref, a_ref), "inverse")
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["bior4.4", "bior3.9"])
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_long_signal_path(engine, name, boundary):
    _long_case(engine, name, boundary, 2, 32768, 5)


@pytest.mark.parametrize("name", ["bior4.4", "bior3.9"])
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_forced_per_level_path(engine, name, boundary):
    with engine.options(VW_FORCE_TILED=1):
        _long_case(engine, name, boundary, 3, 1024, level_cap(get_wavelet(name), 1024))


# ---- 4. single level -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bior1.3", "bior4.4", "bior3.9", "rbio1.5", "rbio4.4"])
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_single_level(engine, name, boundary):
    w = get_wavelet(name)
    for n in (1, 7, 64, 1001):
        x = signals(3, n, 11)
        a_ref, d_ref = R.forward1(x, *analysis(w), boundary)
        a, d = engine.forward1(dev(x), *analysis(w), boundary, 0)
        exact(a, a_ref, f"N={n} approx")
        exact(d, d_ref, f"N={n} detail")
        a_fma, d_fma = R.forward1(x, *analysis(w), boundary, fma=True)
        af, df = engine.forward1(dev(x), *analysis(w), boundary, nat.FLAG_FMA)
        exact(af, a_fma, f"N={n} FMA approx")
        exact(df, d_fma, f"N={n} FMA detail")
        if pairwise_throws(w):
            with pytest.raises(NotImplementedError, match="high-pass"):
                engine.inverse1(a, d, *synthesis(w), boundary, 0)
            continue
        exact(engine.inverse1(a, d, *synthesis(w), boundary, 0), R.inverse1(a_ref, d_ref, *synthesis(w), boundary),
              f"N={n} inverse (high-pass truncated to {len(synthesis(w)[0])} taps)")
        exact(engine.inverse1(a, d, *synthesis(w), boundary, nat.FLAG_FMA),
              R.inverse1(a_ref, d_ref, *synthesis(w), boundary, fma=True), f"N={n} FMA inverse")
        if boundary == O.SYMMETRIC:
            exact(engine.inverse1(a, d, *synthesis(w), boundary, nat.FLAG_BATCH_SYM_INVERSE),
                  R.inverse1(a_ref, d_ref, *synthesis(w), boundary, batch_sym=True), f"N={n} batch inverse")
            exact(engine.inverse1(a, d, *synthesis(w), boundary, nat.FLAG_BATCH_SYM_INVERSE | nat.FLAG_FMA),
                  R.inverse1(a_ref, d_ref, *synthesis(w), boundary, batch_sym=True, fma=True), f"N={n} FMA batch inverse")
    torch.cuda.synchronize()


# ---- 5. guards and the FFT switch ----------------------------------------------------------------------------------
def test_core_levels_guards(engine):
    w = get_wavelet("rbio1.5")   # analysis (2, 10): the cap reads the 2-tap low-pass, the guard both filters
    n = 64
    x = dev(signals(3, n))
    assert O.max_levels(n, 2) == 6
    with pytest.raises(InvalidArgumentException) as e:
        engine.forward(x, *analysis(w), WID_OTHER, O.PERIODIC, 7, nat.FLAG_CORE_LEVELS)
    assert e.value.error_code == ErrorCode.CFG_INVALID_DECOMPOSITION_LEVEL
    with pytest.raises(InvalidArgumentException) as e:   # Lhi_4 = 73 > 64
        engine.forward(x, *analysis(w), WID_OTHER, O.PERIODIC, 4, nat.FLAG_CORE_LEVELS)
    assert e.value.error_code == ErrorCode.VAL_TOO_LARGE
    det, app = engine.forward(x, *analysis(w), WID_OTHER, O.PERIODIC, 3, nat.FLAG_CORE_LEVELS)   # Lhi_3 = 37
    d_ref, a_ref = forward_ref("rbio1.5", O.PERIODIC, 3, n, 3, "f64")
    exact(det, d_ref)
    exact(app, a_ref)
    # the inverse guard, synthesis pair (2, 10) of bior1.5
    b = get_wavelet("bior1.5")
    d4 = torch.zeros((4, 3, n), dtype=torch.float64, device="cuda")
    with pytest.raises(InvalidArgumentException) as e:
        engine.inverse(d4, x, *synthesis(b), WID_OTHER, O.PERIODIC, 4, nat.FLAG_CORE_LEVELS)
    assert e.value.error_code == ErrorCode.VAL_TOO_LARGE
    y = engine.inverse(d4[:3].contiguous(), x, *synthesis(b), WID_OTHER, O.PERIODIC, 3, nat.FLAG_CORE_LEVELS)
    exact(y, R.reconstruct(np.zeros((3, 3, n)), signals(3, n), *synthesis(b), O.PERIODIC))


def test_fft_switch_mixed_level(engine):
    w, n = get_wavelet("bior2.2"), 1500   # analysis (5, 3): level 7 is 257 / 129 taps around N / 8 = 187.5
    x = dev(signals(3, n))
    flags = nat.FLAG_CORE_LEVELS | nat.FLAG_FFT_SWITCH
    with pytest.raises(NotImplementedError, match="level 7"):
        engine.forward(x, *analysis(w), WID_OTHER, O.PERIODIC, 7, flags)
    det, app = engine.forward(x, *analysis(w), WID_OTHER, O.PERIODIC, 5, flags)   # no level mixed, none in the region
    d_ref, a_ref = R.decompose(signals(3, n), *analysis(w), O.PERIODIC, 5, fft=True)
    exact(det, d_ref)
    exact(app, a_ref)
    # without the switch level 7 is an ordinary circular level
    det, app = engine.forward(x, *analysis(w), WID_OTHER, O.PERIODIC, 7, nat.FLAG_CORE_LEVELS)
    d_ref, a_ref = R.decompose(signals(3, n), *analysis(w), O.PERIODIC, 7)
    exact(det, d_ref)
    exact(app, a_ref)


# ---- 6. VW_FLAG_REF_NONFINITE ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bior4.4", "rbio1.5"])
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_ref_nonfinite(engine, name, boundary):
    """One NaN and one +Inf in one row of three: every row bit-exact, NaN positions included, against the full-tap
    restatement (every upsampled tap multiplied, each filter over its own upsampled length)."""
    w, B, n, J = get_wavelet(name), 3, 200, 3
    x = np.array(signals(B, n))
    x[1, 50] = np.nan
    x[1, 140] = np.inf
    d_ref, a_ref = R.decompose_full(x, *analysis(w), boundary, J)
    assert np.isnan(d_ref[:, 1]).any() and np.isfinite(d_ref[:, 0]).all() and np.isfinite(d_ref[:, 2]).all()
    for flags in (nat.FLAG_REF_NONFINITE, nat.FLAG_REF_NONFINITE | nat.FLAG_FMA):
        det, app = engine.forward(dev(x), *analysis(w), WID_OTHER, boundary, J, flags)
        if flags & nat.FLAG_FMA:   # the recomputed row is exact arithmetic also under FMA
            exact(det[:, 1], d_ref[:, 1], "details, flagged row")
            exact(app[1], a_ref[1], "approx, flagged row")
        else:
            exact(det, d_ref, "details")
            exact(app, a_ref, "approx")
    # inverse: clean coefficients with the two values planted in one row
    dc, ac = (np.array(a) for a in forward_ref(name, boundary, B, n, J, "f64"))
    dc[1, 1, 60] = np.nan
    ac[1, 120] = np.inf
    if boundary == O.ZERO_PADDING and pairwise_throws(w):
        with pytest.raises(NotImplementedError, match="high-pass"):
            engine.inverse(dev(dc), dev(ac), *synthesis(w), WID_OTHER, boundary, J, nat.FLAG_REF_NONFINITE)
        return
    y_ref = R.reconstruct_full(dc, ac, *synthesis(w), boundary)
    assert np.isnan(y_ref[1]).any() and np.isfinite(y_ref[0]).all()
    y = engine.inverse(dev(dc), dev(ac), *synthesis(w), WID_OTHER, boundary, J, nat.FLAG_REF_NONFINITE)
    exact(y, y_ref, "inverse")
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["bior3.9", "bior4.4", "rbio1.5"])
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_ref_nonfinite_at_one_level(engine, name, boundary):
    """An equal-length bank has no zero taps at level 1, a zero-extended one has (16 of bior3.9's 20 high-pass
    taps): the fix-up must also run at J = 1 and on the single-level forward, or NaN lands where the reference's
    loops never read."""
    w, B, n = get_wavelet(name), 3, 200
    x = np.array(signals(B, n))
    x[1, 50] = np.nan
    x[1, 140] = np.inf
    d_ref, a_ref = R.decompose_full(x, *analysis(w), boundary, 1)
    for flags in (nat.FLAG_REF_NONFINITE, nat.FLAG_REF_NONFINITE | nat.FLAG_FMA):
        det, app = engine.forward(dev(x), *analysis(w), WID_OTHER, boundary, 1, flags)
        exact(det[:, 1], d_ref[:, 1], "J = 1 details, flagged row")
        exact(app[1], a_ref[1], "J = 1 approx, flagged row")
        a1, d1 = engine.forward1(dev(x), *analysis(w), boundary, flags)
        exact(d1[1], d_ref[0, 1], "forward1 detail, flagged row")
        exact(a1[1], a_ref[1], "forward1 approx, flagged row")
    det, app = engine.forward(dev(x), *analysis(w), WID_OTHER, boundary, 1, nat.FLAG_REF_NONFINITE)
    exact(det, d_ref, "J = 1 details")
    exact(app, a_ref, "J = 1 approx")
    # inverse at one level: the sequential sums run zero-extended filters, the pairwise ones do not
    dc, ac = (np.array(a) for a in forward_ref(name, boundary, B, n, 1, "f64"))
    dc[0, 1, 60] = np.nan
    ac[1, 120] = np.inf
    if boundary == O.ZERO_PADDING and pairwise_throws(w):
        return
    y_ref = R.reconstruct_full(dc, ac, *synthesis(w), boundary)
    y = engine.inverse(dev(dc), dev(ac), *synthesis(w), WID_OTHER, boundary, 1, nat.FLAG_REF_NONFINITE)
    exact(y, y_ref, "J = 1 inverse")
    torch.cuda.synchronize()


# ---- 7. facades ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_multilevel_transform_facade(engine, boundary):
    w, B, n, J = get_wavelet("bior4.4"), 3, 512, 4
    tx = vw.MultiLevelMODWTTransform(w, vw.BoundaryMode(boundary))
    assert tx.getMaximumLevels(n) == O.max_levels(n, 9)
    d_ref, a_ref = forward_ref("bior4.4", boundary, B, n, J, "f64")
    for x in (dev(signals(B, n)), np.array(signals(B, n))):   # device tensors and the host-memory path
        res = tx.decompose(x, J)
        exact(res.details_array, d_ref)
        exact(res.approximation_array, a_ref)
        exact(tx.reconstruct(res), R.reconstruct(d_ref, a_ref, *synthesis(w), boundary))
        exact(tx.reconstructFromLevel(res, 2), R.reconstruct(d_ref, a_ref, *synthesis(w), boundary, 0, 0b1110))
        exact(tx.reconstructLevels(res, 2, 3), R.reconstruct(d_ref, a_ref, *synthesis(w), boundary, 0, 0b0110, True))
    sl = vw.MODWTTransform(w, vw.BoundaryMode(boundary))
    r = sl.forward(np.array(signals(B, n)[0]))
    a1, d1 = R.forward1(signals(B, n)[0], *analysis(w), boundary)
    exact(r.approximationCoeffs(), a1)
    exact(r.detailCoeffs(), d1)
    exact(sl.inverse(r), R.inverse1(a1, d1, *synthesis(w), boundary))


def test_batch_facade(engine):
    w, B, n, J = get_wavelet("bior4.4"), 3, 512, 4
    x = np.array(signals(B, n))
    d_ref, a_ref = forward_ref("bior4.4", O.PERIODIC, B, n, J, "f64")
    ml = vw.BatchMODWT.multiLevelAoS(w, x, J)
    exact(ml.detailPerLevel, d_ref)
    exact(ml.finalApprox, a_ref)
    exact(vw.BatchMODWT.inverseMultiLevelAoS(w, ml.detailPerLevel, ml.finalApprox),
          R.reconstruct(d_ref, a_ref, *synthesis(w), O.PERIODIC))
    sl = vw.BatchMODWT.singleLevelAoS(w, x)
    a1, d1 = R.forward1(x, *analysis(w), O.PERIODIC)
    exact(sl.approx, a1)
    exact(sl.detail, d1)
    exact(vw.BatchMODWT.inverseSingleLevelAoS(w, sl.approx, sl.detail), R.inverse1(a1, d1, *synthesis(w), O.PERIODIC))


@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_swt_adapter_facade(engine, boundary):
    w, n, J = get_wavelet("bior4.4"), 512, 3
    x = np.array(signals(1, n)[0])
    swt = vw.VectorWaveSwtAdapter(w, vw.BoundaryMode(boundary))
    d_ref, a_ref = R.decompose(x, *analysis(w), boundary, J)
    res = swt.forward(x, J)
    exact(res.details_array, d_ref)
    exact(res.approximation_array, a_ref)
    exact(swt.inverse(res), R.reconstruct(d_ref, a_ref, *synthesis(w), boundary))
    exact(swt.extractLevel(x, J, 2), R.reconstruct(d_ref, a_ref, *synthesis(w), boundary, 0, 0b010, True))
    exact(swt.extractLevel(x, J, 0), R.reconstruct(d_ref, a_ref, *synthesis(w), boundary, 0, 0, False))


def test_device_group_refuses_before_any_launch(engine):
    w = get_wavelet("bior4.4")
    x = np.array(signals(2, 256))
    g = vw.DeviceGroup(engines=[engine])   # (the other single-pair facades: tests/test_bior_facades_cpu.py)
    with pytest.raises(NotImplementedError, match="bior4.4"):
        g.forward(x, w, 2)
    with pytest.raises(NotImplementedError, match="bior4.4"):
        g.inverse(np.zeros((2, 2, 256)), x, w)
    with pytest.raises(NotImplementedError, match="bior4.4"):
        g.forward_device([dev(x)], w, 2)
    with pytest.raises(NotImplementedError, match="bior4.4"):
        g.inverse_device([(dev(np.zeros((2, 2, 256))), dev(x))], w)
