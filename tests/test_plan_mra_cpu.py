"""Kernel selection of the multiresolution calls, checked on the CPU: tests/plan_mra_harness links the planner
(vectorwave_amd/csrc/vw_plan.cpp) with nothing from HIP and walks filter lengths 1..64, fp32 / fp64, the three
boundaries, N in {7, 64, 512, 1000, 4096, 8192, 16384, 65536, 2^20}, J from 1 to the level cap (and two past it),
with and without FMA / VALIDATE / REF_NONFINITE, aligned and unaligned pointers, under the default tuning,
VW_MRA_FUSED=0 and =2, VW_FORCE_TILED=1, VW_NV=8, VW_UNROLL_MAX=0 and VW_LEVEL_CT=0.

For each plan:
  - fused: threads are whole waves within k_mra's bound (512 at NV = 4, 1024 at NV = 8) and cover the row, LDS is
    exactly two regions and <= 160 KiB, each region holds the left pad, the row and the longest halos;
  - every level's halos cover the reach of both branches over every output the kernel computes, and an
    owner-written halo lies within the row and the slabs that check it;
  - never fused for a single-level call, VW_FLAG_VALIDATE / VW_FLAG_REF_NONFINITE, VW_FORCE_TILED or VW_MRA_FUSED=0;
    nor, by default, in the class measured slower than the loop (a listed length past kMraUnrollMax on aligned
    full-slab rows, where the inverses have tap-unrolled kernels and k_mra has none; VW_MRA_FUSED=2 fuses there);
    on PERIODIC / ZERO_PADDING, fused wherever two regions fit otherwise;
  - the tap-unrolled body exactly for aligned full-slab rows at a listed length up to kMraUnrollMax;
  - the plan of db4 / J = 6 / 4096 x 4096 / fp64 / PERIODIC is pinned field by field.
The program prints one line per finding and nothing otherwise.

The argument errors of the C ABI that return before any device work are checked here too (no GPU needed).
"""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_mra_harness")
EXE = os.path.join(HERE, "plan_mra_check")
CSRC = os.path.join(HERE, "..", "..", "vectorwave_amd", "csrc")


def _harness():
    srcs = [os.path.join(HERE, f) for f in ("plan_mra_check.cpp", "Makefile")]
    srcs += [os.path.join(CSRC, f) for f in ("vw_plan.cpp", "vw_plan.h", "vw_taps.h", "vw_internal.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in srcs):
        subprocess.run(["make", "-C", HERE, "-s"], check=True)  # normally built by __graft_entry__.build()
    return EXE


def test_every_mra_plan_keeps_its_promises():
    r = subprocess.run([_harness()], capture_output=True, text=True, timeout=300)
    assert r.stdout == "" and r.stderr == "" and r.returncode == 0, r.stdout[-8000:] + r.stderr[-2000:]


# ---- argument errors that return before any device work -------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vectorwave_amd import _native as nat
    return nat.load()


def _taps():
    from vectorwave_amd import _native as nat
    from vectorwave_amd.wavelets import Daubechies
    w = Daubechies.DB4
    return nat.taps_array(w.lowPassDecomposition()), nat.taps_array(w.highPassDecomposition()), len(w.lowPassDecomposition())


FAKE_CTX = ctypes.c_void_p(0x1000)   # non-null, never dereferenced: every case below returns before the context is read
BUF = ctypes.c_void_p(0x2000)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_planes_call_makes_the_inverse_checks(lib, sfx):
    """Same statuses as vw_modwt_inverse_* with every plane kept, for each argument error that needs no device."""
    lo, hi, L = _taps()
    mra = getattr(lib, f"vw_mra_planes_{sfx}")
    inv = getattr(lib, f"vw_modwt_inverse_{sfx}")

    def both(ctx, det, app, B, N, lo_, hi_, L_, boundary, J, flags, out):
        a = mra(ctx, det, app, B, N, lo_, hi_, L_, 0, boundary, J, flags, out)
        b = inv(ctx, det, app, B, N, lo_, hi_, L_, 0, boundary, J, 0xFFFFFFFF, 0, flags, out)
        assert a == b and a != 0, (a, b)
        return a

    seen = set()
    seen.add(both(None, BUF, BUF, 2, 64, lo, hi, L, 0, 2, 0, BUF))        # ctx
    seen.add(both(FAKE_CTX, BUF, BUF, 2, 64, lo, hi, L, 0, 2, 0, None))   # out
    seen.add(both(FAKE_CTX, None, BUF, 2, 64, lo, hi, L, 0, 2, 0, BUF))   # details
    seen.add(both(FAKE_CTX, BUF, None, 2, 64, lo, hi, L, 0, 2, 0, BUF))   # approx
    seen.add(both(FAKE_CTX, BUF, BUF, 2, 64, None, hi, L, 0, 2, 0, BUF))  # taps
    seen.add(both(FAKE_CTX, BUF, BUF, 0, 64, lo, hi, L, 0, 2, 0, BUF))    # empty batch
    seen.add(both(FAKE_CTX, BUF, BUF, 2, 0, lo, hi, L, 0, 2, 0, BUF))     # empty signal
    seen.add(both(FAKE_CTX, BUF, BUF, 2, 64, lo, hi, L, 7, 2, 0, BUF))    # boundary
    seen.add(both(FAKE_CTX, BUF, BUF, 2, 64, lo, hi, 0, 0, 2, 0, BUF))    # filter length
    seen.add(both(FAKE_CTX, BUF, BUF, 2, 64, lo, hi, L, 0, 0, 0, BUF))    # J = 0
    seen.add(both(FAKE_CTX, BUF, BUF, 2, 64, lo, hi, L, 0, 25, 0, BUF))   # J past the engine limit
    seen.add(both(FAKE_CTX, BUF, BUF, 2, 64, lo, hi, L, 0, 5, 1, BUF))    # CORE_LEVELS: L_5 = 113 > 64
    assert len(seen) >= 5   # null, empty, boundary, argument, level, too-large are distinct statuses


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_signal_call_makes_the_forward_checks(lib, sfx):
    """Same statuses as vw_modwt_forward_* for each argument error that needs no device (ldx < N, bad J, boundary)."""
    lo, hi, L = _taps()
    mra = getattr(lib, f"vw_modwt_mra_{sfx}")
    fwd = getattr(lib, f"vw_modwt_forward_{sfx}")

    def both(ctx, x, B, N, ldx, lo_, hi_, L_, boundary, J, flags, out):
        a = mra(ctx, x, B, N, ldx, lo_, hi_, L_, 0, boundary, J, flags, out)
        b = fwd(ctx, x, B, N, ldx, lo_, hi_, L_, 0, boundary, J, flags, out, BUF)
        assert a == b and a != 0, (a, b)
        return a

    seen = set()
    seen.add(both(None, BUF, 2, 64, 64, lo, hi, L, 0, 2, 0, BUF))
    seen.add(both(FAKE_CTX, None, 2, 64, 64, lo, hi, L, 0, 2, 0, BUF))
    seen.add(both(FAKE_CTX, BUF, 2, 64, 64, lo, hi, L, 0, 2, 0, None))
    seen.add(both(FAKE_CTX, BUF, 2, 64, 64, lo, None, L, 0, 2, 0, BUF))
    seen.add(both(FAKE_CTX, BUF, 0, 64, 64, lo, hi, L, 0, 2, 0, BUF))
    seen.add(both(FAKE_CTX, BUF, 2, 64, 63, lo, hi, L, 0, 2, 0, BUF))     # ldx < N
    seen.add(both(FAKE_CTX, BUF, 2, 64, 64, lo, hi, L, 9, 2, 0, BUF))     # boundary
    seen.add(both(FAKE_CTX, BUF, 2, 64, 64, lo, hi, L, 0, 0, 0, BUF))     # J = 0
    seen.add(both(FAKE_CTX, BUF, 2, 64, 64, lo, hi, L, 0, 25, 0, BUF))    # J past the engine limit
    seen.add(both(FAKE_CTX, BUF, 2, 64, 64, lo, hi, L, 0, 5, 1, BUF))     # CORE_LEVELS: J above the cap
    assert len(seen) >= 4


@pytest.mark.parametrize("name", ["vw_mra_planes_f64", "vw_modwt_mra_f64"])
def test_unknown_flags_are_refused(lib, name):
    lo, hi, L = _taps()
    tree_sums = 1 << 9
    if name == "vw_mra_planes_f64":
        st = lib.vw_mra_planes_f64(FAKE_CTX, BUF, BUF, 2, 64, lo, hi, L, 0, 0, 2, tree_sums, BUF)
    else:
        st = lib.vw_modwt_mra_f64(FAKE_CTX, BUF, 2, 64, 64, lo, hi, L, 0, 0, 2, tree_sums, BUF)
    assert st != 0
