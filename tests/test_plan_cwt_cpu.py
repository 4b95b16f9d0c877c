"""Launch shapes of the continuous wavelet transform, checked on the CPU: tests/plan_cwt_harness links the planner
(vectorwave_amd/csrc/vw_plan.cpp) with nothing from HIP and walks tap counts {1, 2, 17, 64, 257, 1201, 8193, 8194,
40000} -- each alone and all of them as one call -- over N in {1, 16, 100, 4096, 65536, 2^20}, fp32 / fp64, real and
complex tables, every extension, B in {1, 300}, with and without FMA.

For each plan:
  - threads are whole waves, at most k_cwt's 256 and at most 1024; the tile is threads x NV with NV = 32 bytes of
    elements; the tiles cover [0, N) exactly once and no wave of a single tile is without outputs;
  - per scale: the staged chunks are the kernel's own rule (cwt_chunks), LDS = chunks x 32 bytes <= 160 KiB, the staged
    span covers every element every computed output reads and every chunk a thread's window loads;
  - the scales run heaviest first (stable), the launches partition that order, a launch's LDS holds each of its
    scales and no scale rides with one needing over twice its LDS beyond the 16 KiB class; grids are within
    1..2^20 and equal the work where it fits;
  - K = 8193 is placed, K = 40000 (any K > 16384) is refused with VW_ERR_UNSUPPORTED naming the scale;
  - the plan of the bench shape (Morlet, 32 log-spaced scales on [1, 128], 256 x 4096, fp64, REFLECT) is pinned
    field by field.
The program prints one line per finding and nothing otherwise.

The argument errors of vw_cwt_f64 / vw_cwt_f32 that return before any device work are checked here too, with a
context pointer that is never dereferenced (no GPU needed).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from vectorwave_amd import errors

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_cwt_harness")
EXE = os.path.join(HERE, "plan_cwt_check")
CSRC = os.path.join(HERE, "..", "..", "vectorwave_amd", "csrc")


def _harness():
    srcs = [os.path.join(HERE, f) for f in ("plan_cwt_check.cpp", "Makefile")]
    srcs += [os.path.join(CSRC, f) for f in ("vw_plan.cpp", "vw_plan.h", "vw_taps.h", "vw_internal.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in srcs):
        subprocess.run(["make", "-C", HERE, "-s"], check=True)  # normally built by __graft_entry__.build()
    return EXE


def test_every_cwt_plan_keeps_its_promises():
    r = subprocess.run([_harness()], capture_output=True, text=True, timeout=300)
    assert r.stdout == "" and r.stderr == "" and r.returncode == 0, r.stdout[-8000:] + r.stderr[-2000:]


# ---- argument errors that return before any device work -------------------------------------------------------
@pytest.fixture(scope="module")
def nat():
    from vectorwave_amd import _native
    _native.load()
    return _native


FAKE_CTX = ctypes.c_void_p(0x1000)   # non-null, never dereferenced: every case below returns before the context is read
BUF = ctypes.c_void_p(0x2000)


def _call(nat, sfx, ctx=FAKE_CTX, x=BUF, B=2, N=64, ldx=64, scales=((0, 17, -8, 1.0),), taps_re="ok", taps_im=None,
          ntaps=40, ext=1, wrap=0, flags=0, out_re=BUF, out_im=BUF, null_scales=False):
    table = (ctypes.c_double * 40)(*([0.25] * 40))
    desc = (nat.CwtScale * max(len(scales), 1))()
    for i, d in enumerate(scales):
        desc[i] = nat.CwtScale(*d)
    fn = getattr(nat.load(), f"vw_cwt_{sfx}")
    return fn(ctx, x, B, N, ldx, None if null_scales else desc, len(scales), table if taps_re == "ok" else None,
              table if taps_im == "ok" else None, ntaps, ext, wrap, flags, out_re, out_im)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_null_and_empty_arguments(nat, sfx):
    assert _call(nat, sfx, ctx=None) == errors.VW_ERR_NULL
    assert _call(nat, sfx, x=None) == errors.VW_ERR_NULL
    assert _call(nat, sfx, out_re=None) == errors.VW_ERR_NULL
    assert _call(nat, sfx, taps_re=None) == errors.VW_ERR_NULL
    assert _call(nat, sfx, null_scales=True) == errors.VW_ERR_NULL
    assert _call(nat, sfx, taps_im="ok", out_im=None) == errors.VW_ERR_NULL   # a complex table needs out_im
    assert _call(nat, sfx, B=0) == errors.VW_ERR_EMPTY
    assert _call(nat, sfx, N=0) == errors.VW_ERR_EMPTY
    assert _call(nat, sfx, scales=()) == errors.VW_ERR_EMPTY


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_argument_errors(nat, sfx):
    bad = errors.VW_ERR_ARG
    assert _call(nat, sfx, ldx=63) == bad                                  # ldx < N
    assert _call(nat, sfx, scales=((0, 0, 0, 1.0),)) == bad                # K_s < 1
    assert _call(nat, sfx, scales=((0, 17, -8, 1.0), (30, 11, -5, 1.0))) == bad   # taps [30, 41) of 40
    assert "scale 1" in nat.last_error()
    assert _call(nat, sfx, scales=((-1, 17, -8, 1.0),)) == bad             # tap_begin < 0
    assert _call(nat, sfx, scales=((0, 17, -8, 0.0),)) == bad              # q_s <= 0
    assert _call(nat, sfx, scales=((0, 17, -8, -2.0),)) == bad
    assert _call(nat, sfx, scales=((0, 17, -8, float("nan")),)) == bad
    assert _call(nat, sfx, ext=5) == bad and _call(nat, sfx, ext=-1) == bad   # unknown extension
    assert _call(nat, sfx, ext=4, wrap=0) == bad                           # WRAP_ZERO without a period
    assert _call(nat, sfx, ntaps=0) == bad
    for flag in (1 << 0, 1 << 1, 1 << 2, 1 << 6, 1 << 8, 1 << 9, 1 << 20):  # anything but FMA, HOST_MEMORY, SYNC
        assert _call(nat, sfx, flags=flag) == bad, flag
    assert "FMA, HOST_MEMORY and SYNC" in nat.last_error()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_a_scale_the_plan_cannot_place_is_named(nat, sfx):
    n = 40000
    table = np.zeros(n + 17)
    desc = (nat.CwtScale * 2)(nat.CwtScale(0, 17, -8, 1.0), nat.CwtScale(17, n, -(n // 2), 1.0))
    fn = getattr(nat.load(), f"vw_cwt_{sfx}")
    tp = table.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    st = fn(FAKE_CTX, BUF, 1, 64, 64, desc, 2, tp, None, table.size, 1, 0, 0, BUF, None)
    assert st == errors.VW_ERR_UNSUPPORTED and "scale 1" in nat.last_error() and "40000" in nat.last_error()
    with pytest.raises(NotImplementedError):
        errors.raise_for_status(st, nat.last_error())
