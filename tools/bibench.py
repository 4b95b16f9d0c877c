#!/usr/bin/env python3
"""Times forward + inverse of biorthogonal banks (vw_modwt_*_bi_*) on one GPU.  A tool, not a test; bench.py is the
project's benchmark and does not know about this.

Configurations (PERIODIC, VW_FLAG_FMA, device tensors):
  bior4.4  J = 6, 4096 x 4096, fp64     analysis (9, 7), synthesis (7, 9): the longer filter's 9 taps are not a listed
                                         tap count
  bior3.9  J = 6, 16384 x 8192, fp32    analysis (20, 4), synthesis (4, 20): 20 taps are listed
  db4      J = 6, 4096 x 4096, fp64     the headline shape, for context

Each bank is timed under six settings in ALTERNATING repeats, `--repeats` each, after one untimed repeat of every
setting:
  default the context's defaults (VW_BI = 3: the two-length route for the pairs with compile-time kernels)
  bi      VW_BI = 7: the two-length route for every pair, in both directions (the non-persistent fused forward and the fused
          sequential inverses run each filter at its own tap count)
  fwd     VW_BI = 1: the two-length forward, the padded inverse
  inv     VW_BI = 2: the padded forward, the two-length inverse
  padded  VW_BI = 0: the padded route, the existing kernels on zero-extended filters (VW_BI_LISTED = 1: one more
          zero tap where that reaches a listed count, the tap-unrolled kernels)
  max     VW_BI = 0, VW_BI_LISTED = 0: max(Llo, Lhi) taps, the runtime-L kernels where that count is unlisted
A repeat is HIP events around `--steps` forward + inverse pairs after `--warmup`, over buffer sets
rotated so that no step re-reads what an earlier one left in the 256 MiB Infinity Cache.  Prints the per-repeat
times, and per configuration and setting the median and the spread (max - min) in milliseconds per pair, then one
JSON line.
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="1/16 of the rows (a quick look)")
    args = ap.parse_args()

    import torch

    import vectorwave_amd as vw
    from vectorwave_amd import _native as nat

    if not torch.cuda.is_available():
        print("bibench needs a GPU (no fallback)", file=sys.stderr)
        return 1
    eng = vw.Engine.get(0)
    SETTINGS = {"default": dict(), "bi": dict(VW_BI=7), "fwd": dict(VW_BI=1), "inv": dict(VW_BI=2),
                "padded": dict(VW_BI=0), "max": dict(VW_BI=0, VW_BI_LISTED=0)}
    ALL = ("default", "bi", "fwd", "inv", "padded", "max")
    configs = [("bior4.4", vw.get_wavelet("bior4.4"), 4096, 4096, torch.float64, ALL),
               ("bior3.9", vw.get_wavelet("bior3.9"), 16384, 8192, torch.float32, ALL),
               ("db4", vw.Daubechies.DB4, 4096, 4096, torch.float64, ("default",))]
    J, flags = 6, nat.FLAG_FMA
    result = {"levels": J, "steps": args.steps, "repeats": args.repeats, "configs": {}}
    for name, w, B, N, dtype, settings in configs:
        if args.small:
            B //= 16
        elem = 8 if dtype == torch.float64 else 4
        sets = max(2, -(-(512 << 20) // (B * N * elem)))
        xs = [eng.fill_uniform(torch.empty((B, N), dtype=dtype, device="cuda"), 42 + i) for i in range(sets)]
        alo, ahi = w.lowPassDecomposition(), w.highPassDecomposition()
        slo, shi = w.lowPassReconstruction(), w.highPassReconstruction()

        def step(i):
            det, app = eng.forward(xs[i % sets], alo, ahi, w.wavelet_id, nat.PERIODIC, J, flags)
            return eng.inverse(det, app, slo, shi, w.wavelet_id, nat.PERIODIC, J, flags)

        def repeat():
            for i in range(args.warmup):
                step(i)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.steps):
                step(args.warmup + i)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.steps

        for s in settings:  # one untimed repeat of each setting first: neither carries a new shape's one-time costs
            with eng.options(**SETTINGS[s]):
                repeat()
        times = {s: [] for s in settings}
        for _ in range(args.repeats):
            for s in settings:
                with eng.options(**SETTINGS[s]):
                    times[s].append(repeat())
        out = {"shape": [B, N], "dtype": str(dtype).replace("torch.", ""), "taps": [len(alo), len(ahi)], "sets": sets}
        for s in settings:
            key = s if len(settings) > 1 else "ms"
            out[key] = {"median_ms": round(statistics.median(times[s]), 4),
                        "spread_ms": round(max(times[s]) - min(times[s]), 4),
                        "repeats_ms": [round(t, 4) for t in times[s]]}
            print(f"{name:8s} {B} x {N} {out['dtype']} {key:9s} median {out[key]['median_ms']:.4f} ms  spread "
                  f"{out[key]['spread_ms']:.4f} ms  {out[key]['repeats_ms']}")
        result["configs"][name] = out
        del xs
        torch.cuda.empty_cache()
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
