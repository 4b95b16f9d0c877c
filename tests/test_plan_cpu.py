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
"""
import os
import subprocess

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
