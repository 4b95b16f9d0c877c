#!/usr/bin/env python3
"""Times the fused financial analysis (vw_fin_analyze_f64) on one GPU.  A tool, not a test; bench.py is the
project's benchmark and does not know about this.

Shape: B price rows of N samples (default 4096 x 4097: 4096 returns per row), geometric random walks.  Four
device times, HIP events around `--steps` back-to-back calls after `--warmup`, buffer sets rotated so that no
step re-reads an input an earlier step left in the 256 MiB Infinity Cache (as bench.py --rotate does):

  exact     vw_fin_analyze_f64, default flags (the reference's sequential sums, bit-identical)
  tree      vw_fin_analyze_f64, VW_FLAG_TREE_SUMS
  composed  the same five outputs from what the engine offered before the fused call: torch computes the
            returns, the single-level forward (the launch MODWTTransform.forwardBatch makes on a device batch,
            Engine.forward1) writes both B x n planes, torch reduces them
  read      torch row sums of the same price buffers: one plain read of the same bytes

Prints a table and one JSON line (times in microseconds per call; exact / tree also as multiples of `read`).
"""
import argparse
import json
import os
import sys
from ctypes import c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--length", type=int, default=4097, help="prices per row (N; N - 1 returns)")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=float, default=3.0, help="anomaly threshold in standard deviations")
    args = ap.parse_args()

    import torch

    import vectorwave_amd as vw
    from vectorwave_amd import _native as nat

    if not torch.cuda.is_available():
        print("finbench needs a GPU (no fallback)", file=sys.stderr)
        return 1
    B, N, K = args.batch, args.length, args.k
    n = N - 1
    w = vw.Daubechies.DB4
    lo, hi = w.lowPassDecomposition(), w.highPassDecomposition()
    tlo, thi = nat.taps_array(lo), nat.taps_array(hi)
    eng = vw.Engine.get(0)
    in_bytes = B * N * 8
    sets = max(2, -(-(512 << 20) // in_bytes))
    gen = torch.Generator(device="cuda").manual_seed(42)
    xs = [100.0 * torch.exp(torch.cumsum(0.01 * torch.randn((B, N), dtype=torch.float64, device="cuda", generator=gen),
                                         dim=1)) for _ in range(sets)]
    outs = [torch.empty((5, B), dtype=torch.float64, device="cuda") for _ in range(sets)]
    eng.bind_torch_stream()

    def fused(flags):
        def step(i):
            x, out = xs[i % sets], outs[i % sets]
            st = eng.lib.vw_fin_analyze_f64(eng.ctx, c_void_p(x.data_ptr()), B, N, N, tlo, thi, len(lo), K, flags,
                                            c_void_p(out.data_ptr()))
            assert st == 0, nat.last_error()
            return out
        return step

    def composed(i):
        p = xs[i % sets]
        p0, p1 = p[:, :-1], p[:, 1:]
        r = torch.where(p0.abs() > 1e-10, (p1 - p0) / p0, torch.zeros((), dtype=p.dtype, device=p.device))
        a, d = eng.forward1(r, lo, hi, 0, 0)
        pos, neg = d > 0, d < 0
        npos, nneg = pos.sum(1), neg.sum(1)
        pa = (d * pos).sum(1) / npos
        na = (-d * neg).sum(1) / nneg
        mx = torch.maximum(pa, na)
        asym = torch.where((npos == 0) | (nneg == 0) | (mx < 1e-10), torch.zeros_like(mx), (na - pa).abs() / mx)
        vol = torch.sqrt((d * d).sum(1) / n)
        trend = (a[:, 1:] - a[:, :-1]).abs().amax(1)
        dev = d - d.mean(1, keepdim=True)
        std = torch.sqrt((dev * dev).sum(1) / n)
        flag = (dev.abs() > (K * std)[:, None]).any(1)
        return torch.stack([asym, vol, trend, flag.to(p.dtype), std])

    def read(i):
        return xs[i % sets].sum(dim=1)

    def time_us(step):
        for i in range(args.warmup):
            step(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            step(args.warmup + i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.steps

    # the three computations agree before anything is timed
    ex, tr, co = fused(0)(0).clone(), fused(nat.FLAG_TREE_SUMS)(0).clone(), composed(0)
    torch.cuda.synchronize()
    assert torch.equal(ex[2], tr[2]) and torch.equal(ex[3], tr[3]) and torch.equal(ex[3], co[3])
    for got in (tr, co):
        assert torch.allclose(got, ex, rtol=1e-10, atol=1e-13), (got - ex).abs().max()

    res = {"shape": [B, N], "sets": sets, "steps": args.steps, "input_mb": in_bytes / 1e6}
    for name, step in (("exact", fused(0)), ("tree", fused(nat.FLAG_TREE_SUMS)), ("composed", composed), ("read", read)):
        res[name + "_us"] = round(time_us(step), 2)
    res["read_gbps"] = round(in_bytes / res["read_us"] / 1e3, 1)
    res["exact_over_read"] = round(res["exact_us"] / res["read_us"], 2)
    res["tree_over_read"] = round(res["tree_us"] / res["read_us"], 2)
    res["composed_over_tree"] = round(res["composed_us"] / res["tree_us"], 2)
    for k in ("exact", "tree", "composed", "read"):
        print(f"{k:9s} {res[k + '_us']:10.1f} us")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
