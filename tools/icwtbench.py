#!/usr/bin/env python3
"""Times the inverse continuous wavelet transform (vw_icwt_*, vw_icwt.hip k_icwt) on one GPU against a torch.fft route
that computes the same sums.  A tool, not a test; bench.py is the project's benchmark and does not know about this.

Shape: Morlet (omega0 = 6), --scales (32) log-spaced scales on [--smin, --smax] = [1, 128], --batch x --length =
256 x 4096 coefficient planes [B][S][N] (M = 4096: the upper scales' tables are capped at 4096 taps); --dtype f64 |
f32.  Device times: HIP events around `--steps` back-to-back calls, buffer sets rotated; one untimed repeat, then
`--repeats` (5) repeats in which the variants alternate; per variant the median and the max - min spread:

  exact   vw_icwt, VW_ICWT_SUM, separate multiply and add
  fma     vw_icwt with VW_FLAG_FMA
  torch   torch.fft: one rfft of the B S rows zero-padded to M, the product with the tables' spectra (the tables laid
          out circularly, weights folded in, transformed once outside the timing), the sum over S, one irfft, a slice
          and the division.  Its output is compared with the kernel's before anything is timed and the agreement
          recorded (torch_rel_err, of max|r|).

Reported: milliseconds; multiply-adds per second (B N sum_j K_j) and, with --valu TFLOPS (the vector FMA rate
tools/valubench measures on the same box for the element type), that rate's share.  --sweep: one scale at a time over
1, 2, 4, ..., 128, kernel against the torch route, to find where the FFT route overtakes the direct kernel.  Prints a
table and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--length", type=int, default=4096)
    ap.add_argument("--scales", type=int, default=32)
    ap.add_argument("--smin", type=float, default=1.0)
    ap.add_argument("--smax", type=float, default=128.0)
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", type=int, default=2, help="rotated buffer sets")
    ap.add_argument("--valu", type=float, default=0.0, help="vector FMA rate of the element type, TFLOP/s (tools/valubench)")
    ap.add_argument("--sweep", action="store_true", help="one scale at a time over 1 .. 128 instead of the scale set")
    args = ap.parse_args()

    import numpy as np
    import torch

    import vectorwave_amd as vw
    from vectorwave_amd import _native as nat
    from vectorwave_amd.cwt import MorletWavelet, ScaleSpace, build_inverse_tables

    if not torch.cuda.is_available():
        print("icwtbench needs a GPU (no fallback)", file=sys.stderr)
        return 1
    B, N = args.batch, args.length
    if N < 128:
        print("icwtbench times the SUM form: --length >= 128", file=sys.stderr)
        return 1
    f32 = args.dtype == "f32"
    dt = torch.float32 if f32 else torch.float64
    eng = vw.Engine.get(0)
    eng.bind_torch_stream()
    wavelet = MorletWavelet()

    def measure(scales):
        S = len(scales)
        t = build_inverse_tables(wavelet, scales, N, 0, S)
        M = t.wrap
        taps = sum(d[1] for d in t.scales)
        cs = [eng.fill_uniform(torch.empty((B, S, N), dtype=dt, device="cuda"), 42 + i) for i in range(args.sets)]

        def kernel(flags):
            def step(i):
                return eng.icwt(cs[i % args.sets], t.scales, t.taps, t.form, t.wrap, t.divisor, flags)
            return step

        # the torch route: descriptor j's table laid out circularly, G_j[(-o_j - k) mod M] = w_j[k], times weight_j
        G = np.zeros((S, M))
        for b0, K, o, plane, weight, _ in t.scales:
            G[plane, (-o - np.arange(K)) % M] = t.taps[b0:b0 + K] * weight
        W = torch.fft.rfft(torch.tensor(G, dtype=dt, device="cuda"), dim=-1)            # [S, M/2+1]

        def torch_route(i):
            X = torch.fft.rfft(cs[i % args.sets], n=M, dim=-1)                          # [B, S, M/2+1]
            return torch.fft.irfft((X * W[None]).sum(dim=1), n=M, dim=-1)[:, :N] / t.divisor

        r = kernel(0)(0)
        tr = torch_route(0)
        err = (r - tr).abs().max().item() / r.abs().max().item()
        assert err <= (1e-9 if not f32 else 1e-3), f"torch route differs from the kernel: {err:.3e} of max|r|"
        del r, tr

        variants = [("exact", kernel(0)), ("fma", kernel(nat.FLAG_FMA)), ("torch", torch_route)]

        def time_ms(step, base):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(args.steps):
                step(base + k)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.steps

        times = {name: [] for name, _ in variants}
        for rep in range(args.repeats + 1):   # repeat 0 is untimed warm-up
            for name, step in variants:
                ms = time_ms(step, rep * args.steps)
                if rep:
                    times[name].append(ms)
        macs = 1.0 * B * N * taps
        res = {"scales": S, "taps": taps, "max_taps": max(d[1] for d in t.scales), "fft_size": M,
               "torch_rel_err": float(f"{err:.2e}")}
        for name, _ in variants:
            ts = times[name]
            res[name + "_ms"] = round(statistics.median(ts), 4)
            res[name + "_spread_ms"] = round(max(ts) - min(ts), 4)
        for name in ("exact", "fma"):
            res[name + "_gmacs"] = round(macs / res[name + "_ms"] / 1e6, 1)
            if args.valu > 0:   # exact spends two instructions per multiply-add: its share counts both
                flops = (2.0 if name == "fma" else 4.0) * macs / (res[name + "_ms"] * 1e-3)
                res[name + "_valu_share"] = round(flops / (args.valu * 1e12), 3)
        res["torch_over_fma"] = round(res["torch_ms"] / res["fma_ms"], 2)
        res["torch_over_exact"] = round(res["torch_ms"] / res["exact_ms"], 2)
        return res

    head = {"shape": [B, N], "dtype": args.dtype, "wavelet": "morlet", "form": "sum", "steps": args.steps,
            "repeats": args.repeats, "sets": args.sets, "valu_tflops": args.valu}
    if args.sweep:
        rows = []
        for s in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0):
            r = measure([s])
            r["scale"] = s
            rows.append(r)
            print(f"scale {s:6.0f}  K {r['max_taps']:5d}  exact {r['exact_ms']:9.4f} ms  fma {r['fma_ms']:9.4f} ms  "
                  f"torch {r['torch_ms']:9.4f} ms  torch/fma {r['torch_over_fma']:.2f}")
        head["sweep"] = rows
    else:
        scales = ScaleSpace.logarithmic(args.smin, args.smax, args.scales).getScales()
        r = measure(scales)
        for name in ("exact", "fma", "torch"):
            extra = f"  {r[name + '_gmacs']:9.1f} GMAC/s" if name != "torch" else ""
            if name != "torch" and args.valu > 0:
                extra += f"  {100 * r[name + '_valu_share']:.1f} % of the vector rate"
            print(f"{name:6s} {r[name + '_ms']:10.4f} ms  (spread {r[name + '_spread_ms']:.4f}){extra}")
        head.update(r)
    print(json.dumps(head))
    return 0


if __name__ == "__main__":
    sys.exit(main())
