"""Kernel selection checked on the CPU: tests/plan_harness links the planner (vectorwave_amd/csrc/vw_plan.cpp)
with nothing from HIP and walks fp32 / fp64 x L = 1..64 x the three boundaries x nine signal lengths x levels x
batch sizes under the default tuning and every option set the GPU tests use, plus flags, misaligned pointers,
padded rows, streaming histories, thresholds, detail masks and single-level calls at seven lengths.

Every plan must respect the launch contracts the kernels state (a kernel without a runtime-L form only at a
listed tap count, LDS and thread limits, the persistent and register-blocked kernels' shapes, level coverage
and buffer ping-pong on the per-level path, probing only by kernels that probe, everything reserved before
the first launch).  The bench configurations, the 512-row headline shard and the filter lengths outside the
unrolled list are pinned as exact plans (tests/plan_harness/pins.inc).  The padded LDS layout of the
register-blocked kernels (blk_pad in vw_internal.h, the one rule the planner and the kernels share) is pinned
as a literal table over vector stride x outputs per thread x tight.  The program prints one line per finding
and nothing otherwise.

Rule 8 of the harness is alignment: a plan that sets a vector-I/O flag (vec_io, unrolled, full), picks the persistent,
register-blocked or matrix-core kernels, or holds a deep step or a step with vec_io must have every caller pointer
that launch touches 16-byte aligned, N a whole number of vectors and, for the forward input, ldx too.  The matrix
moves every caller pointer (x, details, approx, y, thresholds) one element off alone, and all together.

Every transform case of tests/footprint_cases.py goes through `show` under each of its shift patterns: the kernel or
step kinds the table names must be what the planner picks for aligned pointers, and the plan under every pattern must
be the one recorded in tests/golden/footprint_plans.json, so a planner change cannot silently turn a footprint case
into a duplicate of another.
"""
import json
import os
import subprocess

import pytest

import footprint_cases as F

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_harness")
EXE = os.path.join(HERE, "plan_check")
CSRC = os.path.join(HERE, "..", "..", "vectorwave_amd", "csrc")


def _harness():
    srcs = [os.path.join(HERE, f) for f in ("plan_check.cpp", "pins.inc", "Makefile")]
    srcs += [os.path.join(CSRC, f) for f in ("vw_plan.cpp", "vw_plan.h", "vw_taps.h", "vw_internal.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in srcs):
        subprocess.run(["make", "-C", HERE, "-s"], check=True)  # normally built by __graft_entry__.build()
    return EXE


def test_every_plan_respects_the_launch_contracts():
    r = subprocess.run([_harness()], capture_output=True, text=True, timeout=300)
    assert r.stdout == "" and r.stderr == "" and r.returncode == 0, r.stdout[-8000:] + r.stderr[-2000:]


def test_show_prints_one_plan():
    # db4 (8 taps), 4096 x 4096 fp64, J = 6, PERIODIC, VW_FLAG_FMA: the headline forward
    r = subprocess.run([_harness(), "show", "fwd", "f64", "4096", "4096", "8", "6", "0", "8"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("fwd persist threads=512 nv=4 "), r.stdout + r.stderr


def test_show_takes_pointer_offsets_and_ldx():
    base = ["show", "fwd", "f64", "3", "4096", "8", "4", "0", "0"]
    out = {k: subprocess.run([_harness()] + base + v, capture_output=True, text=True, timeout=60).stdout
           for k, v in {"aligned": [], "x": ["x+8"], "d": ["d+8"], "a": ["a+8"], "ldx": ["ldx=4099"]}.items()}
    assert out["aligned"].startswith("fwd persist threads=512 nv=4 ") and out["aligned"].rstrip().endswith(
        "vec_io=1 unrolled=1 full=0")
    for k in ("x", "d", "a", "ldx"):   # the persistent forward has no element form: k_forward_fused's runtime-L body
        assert out[k].startswith("fwd fused threads=512 nv=4 ") and out[k].rstrip().endswith(
            "vec_io=0 unrolled=0 full=0"), (k, out[k])
    inv = ["show", "inv", "f64", "3", "4096", "8", "4", "0", "0"]
    for v in (["d+8"], ["a+8"], ["y+8"], ["d+8", "a+8", "y+8", "t+8"]):
        r = subprocess.run([_harness()] + inv + v, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("vec_io=0 unrolled=0 full=0"), (v, r.stdout)


@pytest.fixture(scope="module")
def recorded():
    with open(F.PLANS_JSON) as f:
        return json.load(f)


def test_the_record_covers_the_table(recorded):
    assert sorted(recorded) == sorted(c.id for c in F.TRANSFORMS)
    for c in F.TRANSFORMS:
        assert sorted(recorded[c.id]) == sorted(F.plan_key(p, m == F.FMA) for m in c.modes for p in c.shift_patterns())


# (in chunks: one `show` process per case, pattern and mode)
@pytest.mark.parametrize("chunk", range(8))
def test_footprint_cases_select_the_kernels_they_name(recorded, chunk):
    exe = _harness()
    for c in F.TRANSFORMS[chunk::8]:
        for mode in c.modes:
            fma = mode == F.FMA
            kinds, text = F.planned(exe, c, "none", fma)   # (planned() also fails on any finding of the rules)
            assert kinds == c.kinds, (c.id, fma, kinds, c.kinds)
            for pattern in c.shift_patterns():
                kinds, text = F.planned(exe, c, pattern, fma)
                assert text == recorded[c.id][F.plan_key(pattern, fma)], (c.id, pattern, fma, text)
                if pattern != "none":  # a shifted pointer of a launch leaves no vector flag set on it
                    assert "unrolled=1" not in text and "full=1" not in text, (c.id, pattern, text)
