"""Kernel selection for banks with two filter lengths, checked on the CPU: tests/plan_bi_harness links the planner
(vectorwave_amd/csrc/vw_plan.cpp) with nothing from HIP and walks the 15 bior and 15 rbio length pairs, both
directions (multi-level and single-level inverse), fp32 / fp64, the three boundaries,
N in {64, 67, 256, 1000, 1024, 1500, 4096, 16384, 32768}, VW_BI in {0, 1, 2, 3, 7}, VW_FORCE_TILED=1 and
VW_BI_LISTED=0, with and without FMA / REF_NONFINITE, and the core decompose's CORE_LEVELS | FFT_SWITCH up to its
level cap.

For each plan:
  - a named kernel runs the pair, LDS <= 160 KiB and threads <= 1024;
  - padded route: one tap count, the longer filter's, or one more where only that count is listed and VW_BI_LISTED
    is on (the low-pass length on the pairwise inverses); it plans as the equal-length call of that tap count;
  - two-length route (VW_BI bit 0: the non-persistent fused forward, bit 1: the fused sequential inverses; bit 2:
    also the pairs without compile-time kernels): taken only by those kernels, at (Llo, Lhi), unrolled only for a
    pair of VW_TAP_PAIR_LIST, and with bit 2 wherever it fits;
  - the halos cover (taps - 1) * s of the longer filter plus the symmetric shifts;
  - the SYMMETRIC orientation is keyed on the low-pass length and the detail branch shifted by tau(Lhi);
  - Lhi = 0 and Lhi = L plan identically;
  - mixed FFT-switch levels and pairwise inverses with Lhi < Llo are refused with the stated errors.
The program prints one line per finding and nothing otherwise.
"""
import os
import subprocess

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_bi_harness")
EXE = os.path.join(HERE, "plan_bi_check")
CSRC = os.path.join(HERE, "..", "..", "vectorwave_amd", "csrc")


def _harness():
    srcs = [os.path.join(HERE, f) for f in ("plan_bi_check.cpp", "Makefile")]
    srcs += [os.path.join(CSRC, f) for f in ("vw_plan.cpp", "vw_plan.h", "vw_taps.h", "vw_internal.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in srcs):
        subprocess.run(["make", "-C", HERE, "-s"], check=True)  # normally built by __graft_entry__.build()
    return EXE


def test_every_two_length_plan_keeps_its_promises():
    r = subprocess.run([_harness()], capture_output=True, text=True, timeout=300)
    assert r.stdout == "" and r.stderr == "" and r.returncode == 0, r.stdout[-8000:] + r.stderr[-2000:]
