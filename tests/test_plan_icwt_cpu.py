"""Launch shapes of the inverse continuous wavelet transform, checked on the CPU: tests/plan_icwt_harness links the
planner (vectorwave_amd/csrc/vw_plan.cpp) with nothing from HIP and walks N in {1, 63, 64, 127, 128, 200, 1024, 1025,
4096, 16384}, fp32 / fp64, table lengths 1 .. 16384 (every length at N = 1025, a list of edge lengths elsewhere, alone
and mixed in one call), B in {1, 300} and a batch past the grid cap, with and without FMA.

For each plan:
  - threads are whole waves, at most k_icwt's 256; the tile is threads x NV with NV = 32 bytes of elements; every
    output of [0, N) is covered exactly once and no wave of a single tile is without outputs;
  - the staged chunks are the kernel's own rule (cwt_chunks) for the call's longest table, LDS = chunks x 32 bytes <=
    160 KiB, and every descriptor's own chunks fit in it, cover every element its outputs read and every chunk a
    thread's window loads;
  - the grid is one workgroup per (row, tile) up to 2^20, the cap beyond (the kernel strides);
  - K = 16384 is placed, K > 16384 is refused with VW_ERR_UNSUPPORTED naming the first such descriptor;
  - the plans of the bench shape (Morlet, 32 log-spaced scales on [1, 128], 256 x 4096, fp64 and fp32) are pinned.
The program prints one line per finding and nothing otherwise.

The argument errors of vw_icwt_f64 / vw_icwt_f32 that return before any device work are checked here too, with a
context pointer that is never dereferenced (no GPU needed).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from vectorwave_amd import errors

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_icwt_harness")
EXE = os.path.join(HERE, "plan_icwt_check")
CSRC = os.path.join(HERE, "..", "..", "vectorwave_amd", "csrc")


def _harness():
    srcs = [os.path.join(HERE, f) for f in ("plan_icwt_check.cpp", "Makefile")]
    srcs += [os.path.join(CSRC, f) for f in ("vw_plan.cpp", "vw_plan.h", "vw_taps.h", "vw_internal.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in srcs):
        subprocess.run(["make", "-C", HERE, "-s"], check=True)  # normally built by __graft_entry__.build()
    return EXE


def test_every_icwt_plan_keeps_its_promises():
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
SUM, DIRECT = 0, 1


def call(nat, sfx, ctx=FAKE_CTX, coef=BUF, B=2, S=3, N=200, ldc=200, scales=((0, 17, -8, 0, 0.5, 1.0),), taps="ok",
         ntaps=40, form=SUM, wrap=256, divisor=3.0, flags=0, out=BUF, ldo=200, null_scales=False, table=None):
    table = (ctypes.c_double * 40)(*([0.25] * 40)) if table is None else table
    desc = (nat.IcwtScale * max(len(scales), 1))()
    for i, d in enumerate(scales):
        desc[i] = nat.IcwtScale(*d)
    fn = getattr(nat.load(), f"vw_icwt_{sfx}")
    return fn(ctx, coef, B, S, N, ldc, None if null_scales else desc, len(scales), table if taps == "ok" else None,
              ntaps, form, wrap, divisor, flags, out, ldo)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_null_and_empty_arguments(nat, sfx):
    assert call(nat, sfx, ctx=None) == errors.VW_ERR_NULL
    assert call(nat, sfx, coef=None) == errors.VW_ERR_NULL
    assert call(nat, sfx, out=None) == errors.VW_ERR_NULL
    assert call(nat, sfx, taps=None) == errors.VW_ERR_NULL
    assert call(nat, sfx, null_scales=True) == errors.VW_ERR_NULL
    assert call(nat, sfx, B=0) == errors.VW_ERR_EMPTY
    assert call(nat, sfx, S=0) == errors.VW_ERR_EMPTY
    assert call(nat, sfx, N=0) == errors.VW_ERR_EMPTY
    assert call(nat, sfx, scales=()) == errors.VW_ERR_EMPTY


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_argument_errors(nat, sfx):
    bad = errors.VW_ERR_ARG
    assert call(nat, sfx, ldc=199) == bad and "ldc" in nat.last_error()
    assert call(nat, sfx, ldo=199) == bad and "ldo" in nat.last_error()
    assert call(nat, sfx, scales=((0, 17, -8, 3, 0.5, 1.0),)) == bad and "plane 3" in nat.last_error()   # plane outside [0, S)
    assert call(nat, sfx, scales=((0, 17, -8, -1, 0.5, 1.0),)) == bad
    assert call(nat, sfx, scales=((0, 0, 0, 0, 0.5, 1.0),)) == bad                      # K_j < 1
    assert call(nat, sfx, scales=((0, 17, -8, 0, 0.5, 1.0), (30, 11, -5, 1, 0.5, 1.0))) == bad   # taps [30, 41) of 40
    assert "scale 1" in nat.last_error()
    assert call(nat, sfx, scales=((-1, 17, -8, 0, 0.5, 1.0),)) == bad                   # tap_begin < 0
    assert call(nat, sfx, ntaps=0) == bad
    for d in (0.0, -2.0, float("nan"), float("inf")):                                   # divisor not > 0 (and finite)
        assert call(nat, sfx, divisor=d) == bad and "divisor" in nat.last_error()
    assert call(nat, sfx, wrap=199) == bad and "wrap" in nat.last_error()               # wrap < N in SUM
    assert call(nat, sfx, wrap=0) == bad
    assert call(nat, sfx, form=2) == bad and call(nat, sfx, form=-1) == bad             # unknown form
    assert "form" in nat.last_error()
    for flag in (1 << 0, 1 << 1, 1 << 2, 1 << 6, 1 << 8, 1 << 9, 1 << 20):              # anything but FMA, HOST_MEMORY, SYNC
        assert call(nat, sfx, flags=flag) == bad, flag
    assert "FMA, HOST_MEMORY and SYNC" in nat.last_error()
    # DIRECT: 2N - 1 taps per descriptor, no FMA, wrap not read
    direct = dict(N=20, ldc=20, ldo=20, form=DIRECT, wrap=0, scales=((0, 39, 0, 0, 0.5, 1.0),))
    assert call(nat, sfx, **dict(direct, scales=((0, 38, 0, 0, 0.5, 1.0),))) == bad and "2N - 1" in nat.last_error()
    assert call(nat, sfx, **dict(direct, flags=1 << 3)) == bad and "VW_FLAG_FMA" in nat.last_error()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_a_table_the_plan_cannot_place_is_named(nat, sfx):
    n = 40000
    table = np.zeros(n + 17)
    tp = table.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    st = call(nat, sfx, scales=((0, 17, -8, 0, 0.5, 1.0), (17, n, -(n // 2), 1, 0.5, 1.0)), table=tp, ntaps=table.size,
              N=64, ldc=64, ldo=64, wrap=64)
    assert st == errors.VW_ERR_UNSUPPORTED and "scale 1" in nat.last_error() and "40000" in nat.last_error()
    with pytest.raises(NotImplementedError):
        errors.raise_for_status(st, nat.last_error())
    # the longest table that is placed passes every check up to the context: the next one is not
    st = call(nat, sfx, scales=((0, 16385, -8192, 0, 0.5, 1.0),), table=tp, ntaps=table.size, N=64, ldc=64, ldo=64, wrap=64)
    assert st == errors.VW_ERR_UNSUPPORTED and "scale 0" in nat.last_error()
