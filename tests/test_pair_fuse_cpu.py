"""The round-trip kernel (vw_pair.hip k_roundtrip) and the planner's pairing predicate, checked without a GPU.

1. pair_fusable (vw_plan.cpp) is a pure host function of two calls and their plans: a small host program
   (tests/pair_fuse_harness) pins which pairs it accepts -- the headline pair, N = 512 and the small batches, and
   nothing that the kernel does not cover, one case per reason.
2. The kernel is compiled for 4 waves per SIMD, so that two 512-thread workgroups share a CU as the persistent
   forward's do: every instantiation (2, 4, 6, 8 taps, FMA and EXACT) must fit 128 VGPRs with no scratch and nothing
   spilled, and uses dynamic LDS only -- the forward's two level regions, whose size for the headline the planner
   reports and the harness' plan bounds below half a CU's 160 KiB.  Read from the compiler's kernel-resource-usage
   remarks, the way tests/test_inverse_waves_cpu.py does; the unit compiles in well under a minute.
"""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "vectorwave_amd", "csrc")
FIELDS = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "SGPRs Spill": "sgpr_spill",
          "VGPRs Spill": "vgpr_spill", "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "static_lds"}

FUSABLE = {"headline", "exact", "n512", "n512_small_batch", "n512_j7", "haar_j1", "padded_rows"}
NOT_FUSABLE = {"other_details", "other_approx", "masked_level", "approx_zero", "ref_nonfinite", "validate",
               "host_memory", "threshold", "y_is_x", "y_in_details", "symmetric", "mixed_modes", "other_batch",
               "other_levels", "sym8", "n4100", "level_ct0", "no_persist", "reverse_walk", "fp32"}


def test_planner_pairs_only_what_the_kernel_covers(tmp_path):
    exe = os.path.join(str(tmp_path), "pair_fuse")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I" + CSRC,
                    "-o", exe, os.path.join(HERE, "pair_fuse_harness", "pair_fuse.cpp"),
                    os.path.join(CSRC, "vw_plan.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True)
    got = dict(line.split(" ", 1) for line in r.stdout.splitlines())
    assert got == {**{k: "1" for k in FUSABLE}, **{k: "0" for k in NOT_FUSABLE}}, r.stdout


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled kernel name: resource usage} of vw_pair.hip, device code only, every tap count."""
    tmp = tmp_path_factory.mktemp("usage")
    r = subprocess.run(["make", "-s", "-C", CSRC, "usage", "U=vw_pair", "EXTRA=--cuda-device-only",
                        f"USAGE_OUT={tmp}/vw_pair.o"], capture_output=True, text=True, timeout=1500)
    out = r.stdout + r.stderr
    found, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = found.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    assert found, out[-4000:]
    return found


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "exact"])
@pytest.mark.parametrize("taps", [2, 4, 6, 8])
def test_roundtrip_kernel_fits_its_register_budget(kernels, taps, fma):
    name = f"k_roundtripIdLi{taps}ELb{int(fma)}EE"
    hits = [v for k, v in kernels.items() if name in k]
    assert len(hits) == 1, (name, sorted(kernels))
    u = hits[0]
    print(name, u)
    assert u["vgprs"] <= 128 and u["occupancy"] >= 4, u
    assert u["scratch"] == 0 and u["sgpr_spill"] == 0 and u["vgpr_spill"] == 0, u
    assert u["static_lds"] == 0, u  # dynamic LDS only: the forward's plan sizes it (next test)


def test_only_the_fp64_short_filters_are_instantiated(kernels):
    names = [k for k in kernels if "k_roundtrip" in k]
    assert len(names) == 8 and all(re.search(r"k_roundtripIdLi[2468]ELb[01]EE", k) for k in names), names


def test_headline_lds_lets_two_workgroups_share_a_cu(tmp_path):
    """The kernel runs in the forward plan's LDS (pair_fusable checks the inverse's halos fit it): for the headline
    that must stay at or below half of a CU's 160 KiB."""
    exe = os.path.join(str(tmp_path), "headline_lds")
    src = os.path.join(str(tmp_path), "lds.cpp")
    with open(src, "w") as f:
        f.write('#include <cstdint>\n#include <cstdio>\n#include "vw_plan.h"\nusing namespace vw;\n'
                'int main() { FwdCall<double> c; c.x = reinterpret_cast<const double*>(uintptr_t(1) << 30);\n'
                'c.details = reinterpret_cast<double*>(uintptr_t(2) << 30); c.approx = reinterpret_cast<double*>'
                '(uintptr_t(4) << 30);\nc.B = 4096; c.N = 4096; c.ldx = 4096; c.L = 8; c.J = 6; c.flags = VW_FLAG_FMA;\n'
                'FwdPlan<double> p; plan_forward(Tuning(), c, &p); printf("%d %d\\n", p.kernel == kFwdPersist, p.lds);'
                ' return 0; }\n')
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17",
                    "-I" + CSRC, "-o", exe, src,
                    os.path.join(CSRC, "vw_plan.cpp")], check=True, timeout=600)
    persist, lds = (int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    print("headline LDS bytes:", lds)
    assert persist == 1 and lds <= 160 * 1024 // 2
