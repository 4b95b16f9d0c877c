"""VW_PAIR_KEEP without a GPU: which round-trip variant the host selects, and what the variants cost in registers.

1. pair_keep_variant (vw_plan.cpp) is a pure host function of the requested value and the three variants' resident
   workgroups per CU: a small host program (tests/pair_keep_harness) pins forced values, clamping, and the auto rule
   with equal and unequal occupancies -- a kept plane is never bought with a resident workgroup.
2. VW_PAIR_KEEP parses as the other switches do: 0, 1, 2 force, larger values clamp to 2, unset or negative is auto.
3. Every variant with kept planes (k_rtrip_keep, KEEP = 1 and 2; 2, 4, 6, 8 taps; FMA and EXACT) fits 128 VGPRs with no
   scratch and nothing spilled: the condition for two 8-wave workgroups per CU.  KEEP = 0 is k_roundtrip, checked
   by tests/test_pair_fuse_cpu.py.
"""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "vectorwave_amd", "csrc")
FIELDS = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "SGPRs Spill": "sgpr_spill",
          "VGPRs Spill": "vgpr_spill", "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "static_lds"}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("pair_keep")), "pair_keep")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I" + CSRC,
                    "-o", exe, os.path.join(HERE, "pair_keep_harness", "pair_keep.cpp"),
                    os.path.join(CSRC, "vw_plan.cpp")], check=True, timeout=600)

    def call(*args, env=None):
        e = {k: v for k, v in os.environ.items() if k != "VW_PAIR_KEEP"}
        e.update(env or {})
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60, check=True, env=e)
        return [int(v) for v in r.stdout.split()]
    return call


def test_limits(harness):
    max_keep, auto_keep, default = harness("limits")
    assert max_keep == 2 and 0 <= auto_keep <= max_keep
    assert default < 0  # auto unless asked


@pytest.mark.parametrize("requested,expect", [(0, 0), (1, 1), (2, 2), (3, 2), (100, 2)])
def test_forced_values_hold_whatever_the_occupancies(harness, requested, expect):
    for occ in ((2, 2, 2), (5, 4, 4), (5, 5, 4), (1, 1, 1)):
        assert harness("rule", requested, *occ) == [expect]


def test_auto_takes_the_most_planes_that_cost_no_workgroup(harness):
    top = harness("limits")[1]
    assert harness("rule", -1, 2, 2, 2) == [top]             # the headline: LDS limits all three alike
    assert harness("rule", -1, 5, 5, 4) == [min(top, 1)]     # the second plane costs a wave per SIMD
    assert harness("rule", -1, 5, 4, 4) == [0]               # already the first one does
    assert harness("rule", -1, 5, 4, 5) == [top]             # each variant is compared with KEEP = 0, not its neighbour
    assert harness("rule", -1, 2, 3, 3) == [top]             # more is no loss either
    assert harness("rule", -7, 5, 5, 4) == harness("rule", -1, 5, 5, 4)


@pytest.mark.parametrize("value,expect", [(0, 0), (1, 1), (2, 2), (3, 2), (-1, None), (-5, None)])
def test_set_option_parsing(harness, value, expect):
    default = harness("limits")[2]
    assert harness("set", value) == [default if expect is None else expect]


@pytest.mark.parametrize("text,expect", [("0", 0), ("1", 1), ("2", 2), ("9", 2), ("-1", None)])
def test_environment_parsing(harness, text, expect):
    default = harness("limits")[2]
    assert harness("env", env={"VW_PAIR_KEEP": text}) == [default if expect is None else expect]
    assert harness("env") == [default]  # unset


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


@pytest.mark.parametrize("keep", [1, 2])
@pytest.mark.parametrize("fma", [True, False], ids=["fma", "exact"])
@pytest.mark.parametrize("taps", [2, 4, 6, 8])
def test_kept_planes_fit_the_register_budget(kernels, taps, fma, keep):
    name = f"k_rtrip_keepIdLi{taps}ELb{int(fma)}ELi{keep}EE"
    hits = [v for k, v in kernels.items() if name in k]
    assert len(hits) == 1, (name, sorted(kernels))
    u = hits[0]
    print(name, u)
    assert u["vgprs"] <= 128 and u["occupancy"] >= 4, u
    assert u["scratch"] == 0 and u["sgpr_spill"] == 0 and u["vgpr_spill"] == 0, u
    assert u["static_lds"] == 0, u


def test_only_two_kept_plane_variants_per_kernel(kernels):
    names = [k for k in kernels if "k_rtrip_keep" in k]
    assert len(names) == 16 and all(re.search(r"k_rtrip_keepIdLi[2468]ELb[01]ELi[12]EE", k) for k in names), names
