#!/usr/bin/env python3
"""Times the multiresolution calls (vw_mra_planes_* / vw_modwt_mra_*) on one GPU against what a caller could do
before them.  A tool, not a test; bench.py is the project's benchmark and does not know about this.

Shapes (--shape): `db4` = db4, J = 6, 4096 x 4096, fp64, PERIODIC; `coif5` = coif5, J = 6, 16384 x 8192 fp32,
PERIODIC; --batch / --length / --levels override.  Device times: HIP events around `--steps` back-to-back calls,
buffer sets rotated so that no step re-reads what an earlier step left in the 256 MiB Infinity Cache.  One untimed
repeat, then `--repeats` (5) repeats in which the variants alternate; per variant the median and the max - min
spread over the repeats:

  planes        vw_mra_planes, default policy (k_mra where the planner fuses)
  planes_loop   vw_mra_planes under VW_MRA_FUSED=0: the J+1 masked inverses
  planes_fused  vw_mra_planes under VW_MRA_FUSED=2: k_mra wherever it fits, also where the policy prefers the loop
  planes_before J+1 vw_modwt_inverse calls with the masks, issued by the caller (what the loop path is, plus the
                C-ABI call overhead)
  signal        vw_modwt_mra, default policy
  signal_before vw_modwt_forward, then J+1 vw_modwt_inverse calls with the masks
  copy          a device copy that moves as many bytes as `planes` must: reads J+1 planes, writes J+1 planes

Prints a table and one JSON line (microseconds per call).
"""
import argparse
import json
import os
import statistics
import sys
from ctypes import c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"db4": ("DB4", 4096, 4096, 6, "f64"), "coif5": ("COIF5", 16384, 8192, 6, "f32")}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=list(SHAPES), default="db4")
    ap.add_argument("--batch", type=int)
    ap.add_argument("--length", type=int)
    ap.add_argument("--levels", type=int)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", type=int, default=0, help="rotated buffer sets (0: enough to pass 512 MiB of input)")
    ap.add_argument("--fma", action="store_true")
    args = ap.parse_args()

    import torch

    import vectorwave_amd as vw
    from vectorwave_amd import _native as nat

    if not torch.cuda.is_available():
        print("mrabench needs a GPU (no fallback)", file=sys.stderr)
        return 1
    wname, B, N, J, dname = SHAPES[args.shape]
    B, N, J = args.batch or B, args.length or N, args.levels or J
    w = getattr(vw.Daubechies if wname.startswith("DB") else vw.Coiflet, wname)
    f32 = dname == "f32"
    dt = torch.float32 if f32 else torch.float64
    lo, hi = w.lowPassDecomposition(), w.highPassDecomposition()
    tlo, thi, L, wid = nat.taps_array(lo), nat.taps_array(hi), len(lo), w.wavelet_id
    eng = vw.Engine.get(0)
    lib, ctx = eng.lib, eng.ctx
    sfx = "f32" if f32 else "f64"
    fwd, inv = getattr(lib, f"vw_modwt_forward_{sfx}"), getattr(lib, f"vw_modwt_inverse_{sfx}")
    planes_fn, signal_fn = getattr(lib, f"vw_mra_planes_{sfx}"), getattr(lib, f"vw_modwt_mra_{sfx}")
    flags = nat.FLAG_FMA if args.fma else 0
    plane_bytes = B * N * (4 if f32 else 8)
    sets = args.sets or max(2, -(-(512 << 20) // ((J + 1) * plane_bytes)))
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731

    xs = [eng.fill_uniform(torch.empty((B, N), dtype=dt, device="cuda"), 42 + i) for i in range(sets)]
    coefs = [torch.empty((J + 1, B, N), dtype=dt, device="cuda") for _ in range(sets)]   # [d_1..d_J, a_J]
    outs = [torch.empty((J + 1, B, N), dtype=dt, device="cuda") for _ in range(sets)]
    scratch = torch.empty((J + 1, B, N), dtype=dt, device="cuda")                        # signal_before's coefficients
    eng.bind_torch_stream()

    def ok(st):
        assert st == 0, nat.last_error()

    def forward(x, c):
        ok(fwd(ctx, P(x), B, N, N, tlo, thi, L, wid, 0, J, flags, P(c), P(c[J])))

    def inverses(c, out):
        for k in range(J + 1):
            ok(inv(ctx, P(c), P(c[J]), B, N, tlo, thi, L, wid, 0, J, (1 << (k - 1)) if k else 0, 1 if k else 0, flags,
                   P(out[k])))

    for x, c in zip(xs, coefs):
        forward(x, c)

    def planes(i):
        c, out = coefs[i % sets], outs[i % sets]
        ok(planes_fn(ctx, P(c), P(c[J]), B, N, tlo, thi, L, wid, 0, J, flags, P(out)))

    def forced(value):
        def step(i):
            eng.set_option("VW_MRA_FUSED", value)
            try:
                planes(i)
            finally:
                eng.set_option("VW_MRA_FUSED", -1)
        return step

    planes_loop, planes_fused = forced(0), forced(2)

    def planes_before(i):
        inverses(coefs[i % sets], outs[i % sets])

    def signal(i):
        ok(signal_fn(ctx, P(xs[i % sets]), B, N, N, tlo, thi, L, wid, 0, J, flags, P(outs[i % sets])))

    def signal_before(i):
        forward(xs[i % sets], scratch)
        inverses(scratch, outs[i % sets])

    def copy(i):
        outs[i % sets].copy_(coefs[i % sets])

    variants = [("planes", planes), ("planes_loop", planes_loop), ("planes_before", planes_before), ("signal", signal),
                ("signal_before", signal_before), ("planes_fused", planes_fused), ("copy", copy)]

    # the computations agree before anything is timed (EXACT: bit for bit)
    planes(0)
    want = outs[0].clone()
    for name, step in variants[1:6]:
        outs[0].zero_()
        step(0)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], want) if not args.fma else torch.allclose(outs[0], want, atol=1e-5), name

    def time_us(step, base):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            step(base + i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.steps

    times = {name: [] for name, _ in variants}
    for rep in range(args.repeats + 1):   # repeat 0 is untimed warm-up
        for name, step in variants:
            t = time_us(step, rep * args.steps)
            if rep:
                times[name].append(t)

    res = {"shape": [B, N], "dtype": dname, "wavelet": wname.lower(), "levels": J, "sets": sets, "steps": args.steps,
           "repeats": args.repeats, "fma": bool(args.fma), "plane_mb": round(plane_bytes / 1e6, 1)}
    for name, _ in variants:
        ts = times[name]
        res[name + "_us"] = round(statistics.median(ts), 1)
        res[name + "_spread_us"] = round(max(ts) - min(ts), 1)
    res["planes_over_copy"] = round(res["planes_us"] / res["copy_us"], 2)
    res["loop_over_planes"] = round(res["planes_loop_us"] / res["planes_us"], 2)
    res["before_over_signal"] = round(res["signal_before_us"] / res["signal_us"], 2)
    res["copy_gbps"] = round(2 * (J + 1) * plane_bytes / res["copy_us"] / 1e3, 1)
    for name, _ in variants:
        print(f"{name:14s} {res[name + '_us']:12.1f} us  (spread {res[name + '_spread_us']:.1f})")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
