"""The footprint cases: one table shared by the CPU pin (tests/test_plan_cpu.py feeds every transform case through
the plan harness' `show`) and the GPU test (tests/test_gpu_footprint.py runs every case on guarded arenas,
tests/guarded.py).

A case names the entry point (a builder of tests/host_calls.py), the filter, the element type, B, N, the leading
dimension of a row input, J, the boundary, extra flags, the context switches, the kernel (with its vectors per
thread, "persist/4") or the per-level step kinds in launch order it exists for when every pointer is 16-byte aligned
(`kinds`), and the launch family `engine.kernel_time` must count on the GPU.  What the planner picks under each shift
pattern -- a shifted pointer makes it leave the vector kernels: the persistent, register-blocked and matrix-core
forwards fall back to k_forward_fused, the deep steps to column sweeps -- is recorded per case and pattern in
tests/golden/footprint_plans.json (`PYTHONPATH=. python tests/footprint_cases.py` rewrites it from the plan harness; review the
difference like any other change of a pin).  Every case runs with flags 0 and VW_FLAG_FMA unless `modes` says
otherwise.  The shapes are the smallest at which each form exists: the ones the existing tests use to reach it.

Shift patterns: "none", "all", and every device pointer of the call alone ("x", "details", ...: the names the
builders give their arrays, in order of creation)."""
import json
import os
import re
import subprocess
from dataclasses import dataclass

from oracle import oracle as O
from vectorwave_amd import _native as nat
from vectorwave_amd.wavelets import get_wavelet

import host_calls as H
import restatement_generic as G

P, S, Z = nat.PERIODIC, nat.SYMMETRIC, nat.ZERO_PADDING
BNAME = {P: "P", S: "S", Z: "Z"}
EXACT, FMA = 0, nat.FLAG_FMA
BOTH = (EXACT, FMA)


def bank(name):
    """A catalogue wavelet, or "synL": the synthetic L-tap bank of restatement_generic (analysis = synthesis)."""
    if name.startswith("syn"):
        lo, hi = G.synthetic_filter(int(name[3:]))
        return H.Bank(lo, hi)
    return get_wavelet(name)


def taps_of(w):
    return max(len(w.lowPassDecomposition()), len(w.highPassDecomposition()))


def level_cap(name, n, want=4):
    return min(want, O.max_levels(n, taps_of(bank(name))))


@dataclass(frozen=True)
class Case:
    id: str
    entry: str                 # H.CALLS / H.MORE_CALLS key, or a name test_gpu_footprint.py runs itself
    wavelet: str = "db4"
    dtype: str = "f64"
    B: int = 3
    N: int = 64
    ld: int = 0                # 0: the entry point takes no leading dimension (or N)
    J: int = 1
    boundary: int = P
    flags: int = 0
    opts: tuple = ()           # ((switch, value), ...)
    kinds: tuple = ()          # plan harness names, aligned: ("persist/4",) or the per-level steps in launch order
    family: str = ""           # "forward" / "forward_level" / "inverse" / "inverse_level": the launches counted
    modes: tuple = BOTH
    pointers: tuple = ()       # device pointers in order of creation
    patterns: tuple = ()       # () = none, all and every pointer alone
    extra: tuple = ()          # ((keyword, value), ...) for the builder: detail_mask, approx_zero, method ...

    def shift_patterns(self):
        return self.patterns or ("none", "all") + self.pointers

    def shifts(self, pattern):
        return pattern if pattern in ("none", "all") else {self.pointers.index(pattern)}

    def is_transform(self):
        return self.family != ""


FWD_PTRS = ("x", "details", "approx")
INV_PTRS = ("details", "approx", "y")


def _fwd(id, **kw):
    dt = kw.get("dtype", "f64")
    bi = kw.pop("bi", False)
    kw.setdefault("ld", kw.get("N", 64))
    kw.setdefault("family", "forward")
    return Case(id=id, entry=f"vw_modwt_forward_{'bi_' if bi else ''}{dt}", pointers=FWD_PTRS, **kw)


def _inv(id, **kw):
    dt = kw.get("dtype", "f64")
    bi = kw.pop("bi", False)
    kw.setdefault("family", "inverse")
    kw.setdefault("pointers", INV_PTRS)
    return Case(id=id, entry=f"vw_modwt_inverse_{'bi_' if bi else ''}{dt}", **kw)


# ---- forward ----------------------------------------------------------------------------------------------------
FORWARD = []
# k_forward_fused, small rows: every N mod 4 class that matters, three boundaries, packed and padded rows; the
# validating and the fix-up forms of each.  Padded or odd rows run the runtime-L body (no vector I/O).
for _n in (64, 67, 258):
    for _b in (P, S, Z):
        for _pad in (0, 3, 8):
            for _fl, _fn in ((0, ""), (nat.FLAG_VALIDATE, "-validate"), (nat.FLAG_REF_NONFINITE, "-refnf")):
                FORWARD.append(_fwd(f"fwd-small-{_n}-{BNAME[_b]}-ld{_pad}{_fn}", N=_n, ld=_n + _pad, boundary=_b,
                                    J=level_cap("db4", _n), flags=_fl, kinds=("fused/4",)))
            if _pad != 8:
                FORWARD.append(_fwd(f"fwd-small-f32-{_n}-{BNAME[_b]}-ld{_pad}", dtype="f32", N=_n, ld=_n + _pad,
                                    boundary=_b, J=level_cap("db4", _n), kinds=("fused/4",)))
FORWARD += [
    # NV = 8, more than 64 KiB of LDS
    _fwd("fwd-fused-nv8", N=8192, J=4, opts=(("VW_FWD_PERSIST", 0),), kinds=("fused/8",)),
    # k_forward_persist; a shifted pointer falls back to k_forward_fused
    _fwd("fwd-persist", N=4096, J=4, kinds=("persist/4",)),
    _fwd("fwd-persist-f32", dtype="f32", N=4096, J=4, kinds=("persist/4",)),
    # (B = 2 x resident grid + 5 at N = 512: test_gpu_footprint.py sets B, the plan does not depend on it)
    _fwd("fwd-persist-rows", N=512, J=2, B=-1, kinds=("persist/4",), patterns=("none", "all", "x")),
    # k_forward_blk and its VW_BLK_FWD8 = 0 sibling
    _fwd("fwd-blk", wavelet="db8", N=8192, J=4, kinds=("blk/8",)),
    _fwd("fwd-blk-fwd8-0", wavelet="db8", N=8192, J=4, opts=(("VW_BLK_FWD8", 0),), kinds=("fused/8",)),
    # runtime-L bodies
    _fwd("fwd-syn9", wavelet="syn9", N=1000, J=level_cap("syn9", 1000), kinds=("fused/4",)),
    _fwd("fwd-syn22", wavelet="syn22", N=1000, J=level_cap("syn22", 1000), kinds=("fused/4",)),
    # NV = 2
    _fwd("fwd-nv2", N=4096, J=4, opts=(("VW_FWD_NV", 2),), kinds=("fused/2",)),
    # per-level path
    _fwd("fwd-tiled", N=8192, J=4, opts=(("VW_FORCE_TILED", 1),), kinds=("multi",), family="forward_level"),
    _fwd("fwd-tiled-multi0", N=8192, J=4, opts=(("VW_FORCE_TILED", 1), ("VW_MULTI", 0)),
         kinds=("tile", "tile", "tile", "deep"), family="forward_level"),
    # long signals
    _fwd("fwd-long", wavelet="db8", B=2, N=1 << 15, J=10, kinds=("multi", "deep"), family="forward_level"),
    _fwd("fwd-long-deep1", wavelet="db8", B=2, N=1 << 15, J=10, opts=(("VW_DEEP", 1),), kinds=("multi", "deep"), family="forward_level"),
    _fwd("fwd-long-deep0", wavelet="db8", B=2, N=1 << 15, J=10, opts=(("VW_DEEP", 0),),
         kinds=("multi", "sweep", "sweep", "sweep", "sweep", "sweep"), family="forward_level"),
    _fwd("fwd-long-30000", wavelet="db8", B=2, N=30000, J=10,
         kinds=("multi", "sweep", "sweep", "sweep", "sweep", "sweep"), family="forward_level"),
    # matrix cores: fp32 FMA, the smallest case of tests/test_gpu_mfma.py
    _fwd("fwd-mfma", wavelet="db8", dtype="f32", B=1, N=2048, J=1, opts=(("VW_MFMA", 3),), modes=(FMA,),
         kinds=("mfma/4",)),
]
# two lengths: a compile-time pair, and a pair on the runtime-L two-length bodies
for _n in (258, 1000):
    FORWARD.append(_fwd(f"fwd-bior4.4-{_n}", bi=True, wavelet="bior4.4", N=_n, J=level_cap("bior4.4", _n),
                        kinds=("fused/4",)))
    FORWARD.append(_fwd(f"fwd-bior3.9-{_n}", bi=True, wavelet="bior3.9", N=_n, J=level_cap("bior3.9", _n),
                        opts=(("VW_BI", 7),), kinds=("fused/4",)))

# ---- inverse (inputs: the restatement's coefficients) -----------------------------------------------------------
INVERSE = [
    # pair form: one level, ZERO_PADDING
    _inv("inv-pair-8192", N=8192, J=1, boundary=Z, kinds=("pair/8",)),
    _inv("inv-pair-67", N=67, J=1, boundary=Z, kinds=("pair/4",)),
    Case(id="inv1-pair-8192", entry="vw_modwt1_inverse_f64", N=8192, J=1, boundary=Z, kinds=("pair/8",),
         family="inverse", pointers=("approx", "detail", "y")),
    Case(id="inv1-pair-67", entry="vw_modwt1_inverse_f64", N=67, J=1, boundary=P, kinds=("pair/4",),
         family="inverse", pointers=("approx", "detail", "y")),
    _inv("inv-db", N=8192, J=4, opts=(("VW_INV_BUF", 2),), kinds=("db/8",)),
    _inv("inv-seq-sym", N=8192, J=4, boundary=S, opts=(("VW_INV_BUF", 1),), kinds=("seq/8",)),
    _inv("inv-blk", wavelet="db8", N=8192, J=4, kinds=("blk/8",)),
    _inv("inv-full-w6", N=4096, J=4, opts=(("VW_INV_BUF", 1), ("VW_INV_WAVES", 6)), kinds=("seq/4",)),
    _inv("inv-full-w8", N=4096, J=4, opts=(("VW_INV_BUF", 1), ("VW_INV_WAVES", 8)), kinds=("seq/4",)),
    _inv("inv-full-f32", dtype="f32", N=4096, J=4, opts=(("VW_INV_BUF", 1),), kinds=("seq/4",)),
    _inv("inv-multi-ni4", N=8192, J=4, opts=(("VW_FORCE_TILED", 1), ("VW_MULTI_NI", 4)), kinds=("multi",),
         family="inverse_level"),
    _inv("inv-multi-ni8", N=8192, J=4, opts=(("VW_FORCE_TILED", 1), ("VW_MULTI_NI", 8), ("VW_MULTI_INV_TILE", 3968)),
         kinds=("multi",), family="inverse_level"),
    # masks: reconstructLevels / reconstructFromLevel shapes on one fused and one per-level case
    _inv("inv-mask-fused", N=4096, J=5, extra=(("detail_mask", 0x15),), kinds=("db/4",)),
    _inv("inv-az-fused", N=4096, J=5, extra=(("approx_zero", 1), ("app", False)), kinds=("db/4",),
         pointers=("details", "y")),
    _inv("inv-mask-tiled", N=8192, J=5, opts=(("VW_FORCE_TILED", 1),), extra=(("detail_mask", 0x15),),
         kinds=("multi",), family="inverse_level"),
    _inv("inv-az-tiled", N=8192, J=5, opts=(("VW_FORCE_TILED", 1),), extra=(("approx_zero", 1), ("app", False)),
         kinds=("multi",), family="inverse_level", pointers=("details", "y")),
]
# column sweeps (single, chained pairs, chained triples) and the deep inverse
_SW = (("VW_SWEEP2_MINB", 1),)
for _g, _k in ((3, ("sweepg", "sweepg", "multi")), (2, ("sweepg", "sweepg", "sweep", "multi")),
               (0, ("sweep", "sweep", "sweep", "sweep", "sweep", "multi"))):
    INVERSE.append(_inv(f"inv-sweep2-{_g}", wavelet="db8", B=2, N=1 << 15, J=10, opts=_SW + (("VW_SWEEP2", _g),),
                        kinds=_k, family="inverse_level"))
INVERSE += [
    _inv("inv-sweep-3x2p14", B=2, N=3 << 14, J=10, opts=_SW, kinds=("sweepg", "sweep", "multi"),
         family="inverse_level"),
    _inv("inv-deep", wavelet="db8", B=2, N=1 << 15, J=10, opts=_SW + (("VW_DEEP_INV", 1),), kinds=("sweep", "sweep", "deep", "deep", "multi"),
         family="inverse_level"),
]

# two lengths, as the forward: the compile-time pair and the runtime-L two-length bodies
INVERSE += [
    _inv("inv-bior4.4-258", bi=True, wavelet="bior4.4", N=258, J=level_cap("bior4.4", 258), kinds=("db/4",)),
    _inv("inv-bior3.9-1000", bi=True, wavelet="bior3.9", N=1000, J=level_cap("bior3.9", 1000), opts=(("VW_BI", 7),),
         kinds=("db/4",)),
]

TRANSFORMS = FORWARD + INVERSE
assert len({c.id for c in TRANSFORMS}) == len(TRANSFORMS)


def show_args(case, pattern, fma):
    """argv of `plan_check show` for a transform case under a shift pattern."""
    w = bank(case.wavelet)
    inverse = "inverse" in case.entry
    lo = w.lowPassReconstruction() if inverse else w.lowPassDecomposition()
    hi = w.highPassReconstruction() if inverse else w.highPassDecomposition()
    elem = 8 if case.dtype == "f64" else 4
    extra = dict(case.extra)
    argv = ["show", "inv" if inverse else "fwd", case.dtype, str(max(case.B, 3)), str(case.N), str(len(lo)),
            str(case.J), str(case.boundary), hex(case.flags | (nat.FLAG_FMA if fma else 0)), str(w.wavelet_id)]
    argv += [f"{k}={v}" for k, v in case.opts]
    if len(hi) != len(lo):
        argv.append(f"Lhi={len(hi)}")
    if "modwt1" in case.entry:
        argv.append("single=1")
    if not inverse:
        argv.append(f"ldx={case.ld}")
    if "detail_mask" in extra:
        argv.append(f"mask={extra['detail_mask']:#x}")
    if extra.get("approx_zero"):
        argv.append("az=1")
    letter = {"x": "x", "details": "d", "detail": "d", "approx": "a", "y": "y"}
    for name in case.pointers:
        if pattern == "all" or pattern == name:
            argv.append(f"{letter[name]}+{elem}")
    return argv


# ---- the recorded plans ---------------------------------------------------------------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))
PLANS_JSON = os.path.join(HERE, "golden", "footprint_plans.json")


def plan_summary(show_stdout):
    """(kinds, text) of one `show` line: the kernel with its vectors per thread or the step kinds, and the same with
    the flags that choose between the vector and the element forms ("persist/4 vec_io=1 unrolled=1 full=0",
    "multi deep vec_io=[1 1]")."""
    line = show_stdout.splitlines()[0]
    if " levels:" in line:
        kinds = tuple(re.findall(r" (\w+)\[\d", line))
        return kinds, " ".join(kinds) + " " + line[line.rindex("vec_io="):]
    kinds = (line.split()[1] + "/" + re.search(r" nv=(\d+)", line).group(1),)
    return kinds, kinds[0] + " " + line[line.rindex("vec_io="):]


def plan_key(pattern, fma):
    return pattern + ("/fma" if fma else "")


def planned(exe, case, pattern, fma):
    r = subprocess.run([exe] + show_args(case, pattern, fma), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (case.id, pattern, r.stdout + r.stderr)
    return plan_summary(r.stdout)


def record(exe):
    out = {}
    for c in TRANSFORMS:
        out[c.id] = {plan_key(pat, m == FMA): planned(exe, c, pat, m == FMA)[1]
                     for m in c.modes for pat in c.shift_patterns()}
    with open(PLANS_JSON, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    record(os.path.join(HERE, "plan_harness", "plan_check"))
