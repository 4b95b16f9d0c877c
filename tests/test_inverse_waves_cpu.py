"""The register budget of k_inverse_seq's PLAIN form, checked without a GPU.

VW_INV_WAVES=8 only pays if the 8-wave instantiation really fits 64 VGPRs with nothing spilled: four 512-thread
workgroups per CU need 8 waves per SIMD, and a kernel that reaches the cap by spilling trades the occupancy for
scratch traffic.  The test compiles the two vw_inv units (fp64, fp32) for gfx950 the way `make usage` does
(device code only, the 8-tap kernels: DEV_TAPS='X(8)') and reads the compiler's kernel-resource-usage remarks;
the two compilations run side by side and take two to three minutes.  A second test links the planner into a
small host program (tests/plan_waves_harness) and pins which calls it marks for the PLAIN form.
"""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vectorwave_amd", "csrc")
FIELDS = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "SGPRs Spill": "sgpr_spill",
          "VGPRs Spill": "vgpr_spill", "Occupancy [waves/SIMD]": "occupancy"}


def usage(elem, tmp_path):
    """{mangled kernel name: {vgprs, scratch, sgpr_spill, vgpr_spill, occupancy}} of vw_inv.hip at -DVW_T=elem."""
    r = subprocess.run(["make", "-s", "-C", CSRC, "usage", "U=vw_inv", f"T={elem}", "DEV_TAPS=X(8)",
                        "EXTRA=--cuda-device-only", f"USAGE_OUT={tmp_path}/vw_inv_{elem}.o"],
                       capture_output=True, text=True, timeout=1500)
    out = r.stdout + r.stderr
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    assert kernels, out[-4000:]
    return kernels


# k_inverse_seq<T, 8, FMA, 4, true, 8, W, true>: the PLAIN full-slab form of the 8-tap kernel
def plain_name(elem, fma, waves):
    return f"k_inverse_seqI{elem}Li8ELb{int(fma)}ELi4ELb1ELi8ELi{waves}ELb1EE"


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    """Both units, compiled side by side (a couple of minutes each)."""
    from concurrent.futures import ThreadPoolExecutor
    tmp = tmp_path_factory.mktemp("usage")
    with ThreadPoolExecutor(2) as pool:
        jobs = {elem: pool.submit(usage, elem, tmp) for elem in ("double", "float")}
        return {elem: job.result() for elem, job in jobs.items()}


@pytest.fixture(scope="module")
def f64(units):
    return units["double"]


def one(kernels, part):
    hits = [v for k, v in kernels.items() if part in k]
    assert len(hits) == 1, (part, [k for k in kernels if "k_inverse_seq" in k])
    return hits[0]


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "exact"])
def test_eight_wave_plain_form_fits_64_vgprs_without_spills(f64, fma):
    u = one(f64, plain_name("d", fma, 8))
    print(u)
    assert u["vgprs"] <= 64 and u["occupancy"] >= 8, u
    assert u["scratch"] == 0 and u["sgpr_spill"] == 0 and u["vgpr_spill"] == 0, u


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "exact"])
def test_six_wave_plain_form_has_no_scratch(f64, fma):
    u = one(f64, plain_name("d", fma, 6))
    print(u)
    assert u["vgprs"] <= 80 and u["scratch"] == 0 and u["sgpr_spill"] == 0 and u["vgpr_spill"] == 0, u


def test_planner_marks_only_plain_calls(tmp_path):
    """The planner (host-only, plain C++ compiler) sets InvArgs::plain for the full-slab fp64 PERIODIC
    reconstruction from every plane and for nothing else, whatever VW_INV_WAVES says; the switch takes 6 or 8."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = os.path.join(str(tmp_path), "plan_waves")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I" + CSRC,
                    "-o", exe, os.path.join(here, "plan_waves_harness", "plan_waves.cpp"),
                    os.path.join(CSRC, "vw_plan.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True)
    got = dict(line.split(" ", 1) for line in r.stdout.splitlines())
    assert got == {
        "default": "seq full=1 plain=1 waves=6",
        "waves8": "seq full=1 plain=1 waves=8",
        "waves7": "seq full=1 plain=1 waves=6",
        "exact": "seq full=1 plain=1 waves=8",
        "small_db": "db full=1 plain=0 waves=8",
        "small_seq": "seq full=1 plain=1 waves=8",
        "n1024_j7": "seq full=1 plain=1 waves=8",
        "threshold": "seq full=1 plain=0 waves=8",
        "symmetric": "seq full=1 plain=0 waves=8",
        "ragged": "seq full=0 plain=0 waves=8",
        "approx_zero": "seq full=1 plain=0 waves=8",
        "masked_level": "seq full=1 plain=0 waves=8",
        "ref_nonfinite": "seq full=1 plain=0 waves=8",
        "reverse_walk": "seq full=1 plain=0 waves=8",
        "level_ct0": "seq full=0 plain=0 waves=8",
        "misaligned": "seq full=0 plain=0 waves=8",
        "taps16": "other full=1 plain=0 waves=8",
        "fp32": "seq full=1 plain=0 waves=8",
    }, r.stdout


def test_fp32_unit_has_no_plain_form(units):
    """The PLAIN form is fp64 only (vw_inv.hip): the fp32 unit keeps the general full-slab form alone."""
    k = units["float"]
    assert not [n for n in k if re.search(r"k_inverse_seqIfLi8ELb[01]ELi4ELb1ELi8ELi[68]ELb1EE", n)]
    assert any("k_inverse_seqIfLi8E" in n for n in k)
