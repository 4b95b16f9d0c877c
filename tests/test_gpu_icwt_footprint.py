"""Where vw_icwt_* reads and writes: the coefficient planes and the output rows each live alone inside a guarded arena
(tests/guarded.py), as tests/test_gpu_footprint.py does for the other calls.

For k_icwt (SUM form, N = 200 and 1025: a zero region, and a second tile with one live output in fp64) and
k_icwt_direct (N = 5 and 127), fp64 and fp32, padded rows on both sides (ldc = N + 3, ldo = N + 1, the pad elements at
the sentinel), under the pointer patterns
    none      coef and out 16-byte aligned
    coef      coef one element off a 16-byte boundary
    out       out one element off
    all       both off
no guard, pad or input word changes, every output element is written, and the payload is the restatement's bits
(tests/icwt_restatement.py); with VW_FLAG_FMA (SUM form) the fused restatement's."""
import ctypes

import numpy as np
import pytest

import guarded
import icwt_restatement as R
from vectorwave_amd import _native as nat
from vectorwave_amd.cwt import MorletWavelet, build_inverse_tables, next_power_of_two

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32}
B, S = 3, 4
PATTERNS = {"none": "none", "coef": {0}, "out": {1}, "all": "all"}


def _case(N):
    """Tables over planes 1..3 of 4 (plane 0 is never read) and the planes [B][S][ldc] with their padding mask."""
    M = next_power_of_two(N)
    scales = [0.02, 0.16, 1.0, M / 32.0] if N >= 128 else [0.5, 1.0, 2.5, 7.0]
    return build_inverse_tables(MorletWavelet(), sorted(scales), N, 1, S)


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N", [5, 127, 200, 1025])
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_icwt_footprint(engine, dname, N):
    import torch
    dt = NP[dname]
    t = _case(N)
    ldc, ldo = N + 3, N + 1
    count = (B * S - 1) * ldc + N                      # the last row's padding need not exist
    flat = np.random.default_rng(N).standard_normal(count).astype(dt)
    pad = (np.arange(count) % ldc) >= N
    planes = np.zeros((B, S, ldc), dtype=dt)
    planes.reshape(-1)[:count] = flat                  # what the restatement may see: the data alone
    planes[:, :, N:] = 0
    desc = (nat.IcwtScale * len(t.scales))(*[nat.IcwtScale(int(a), int(k), int(o), int(p), float(w), float(s))
                                             for a, k, o, p, w, s in t.scales])
    fn = engine.lib.vw_icwt_f64 if dt == np.float64 else engine.lib.vw_icwt_f32
    engine.bind_torch_stream()
    for fma in ((False, True) if t.form == nat.ICWT_SUM else (False,)):
        want = R.reconstruct_rows(planes, N, t, dt, fma)
        assert not guarded.holds_sentinel(want)
        for pname, shifts in PATTERNS.items():
            side = guarded.GuardedSide(torch, N, shifts)
            coef = side._new("coef", "in", flat, pad)
            opad = (np.arange((B - 1) * ldo + N) % ldo) >= N
            out = side._new("out", "out", np.zeros((B - 1) * ldo + N, dt), opad)
            dp = ctypes.cast(ctypes.c_void_p(side.structs(desc, name="scales")), ctypes.POINTER(nat.IcwtScale))
            st = fn(engine.ctx, ctypes.c_void_p(coef.ptr), B, S, N, ldc, dp, len(t.scales), side.table(t.taps, "taps"),
                    t.taps.size, t.form, t.wrap, t.divisor, side.flags | (nat.FLAG_FMA if fma else 0),
                    ctypes.c_void_p(out.ptr), ldo)
            assert st == 0, (pname, st, nat.last_error())
            guarded.check(side)
            assert coef.ptr % 16 == (dt().itemsize if pname in ("coef", "all") else 0)
            assert out.ptr % 16 == (dt().itemsize if pname in ("out", "all") else 0)
            got = guarded.row_matrix(out.payload(), B, N, ldo)
            assert _bits(got, want), f"{dname} N={N} fma={fma} [{pname}]"
