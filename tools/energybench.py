#!/usr/bin/env python3
"""Times the batch wavelet energies (vw_modwt_energy_f64) on one GPU.  A tool, not a test; bench.py is the
project's benchmark and does not know about this.

Shape: B x N fp64 (default 4096 x 4096), db4, J = 6, PERIODIC.  Device times, HIP events around `--steps`
back-to-back calls after `--warmup`, buffer sets rotated so that no step re-reads an input an earlier step left in
the 256 MiB Infinity Cache (as bench.py --rotate does):

  exact     vw_modwt_energy_f64, default flags: forward into the context workspace, then the sequential chain
            walk over its planes (the reference's sums, bit-identical)
  tree      vw_modwt_energy_f64, VW_FLAG_TREE_SUMS: the fused energy kernel (x read once, (J+1)*B doubles written)
  composed  what a user could do before: Engine.forward, then torch (c*c).sum(-1) per plane
  read      torch row sums of the same x buffers: one plain read of the input bytes
  host      (once, not in the loop) the path `exact` replaces: copy the planes to the host and run
            np.add.accumulate(c*c) per row, as vectorwave_amd.modwt._energy does

Prints a table and one JSON line (times in microseconds per call, `host` in milliseconds).
"""
import argparse
import json
import os
import sys
import time
from ctypes import c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--length", type=int, default=4096)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=256, help="rows of the host path that are timed (scaled to B)")
    args = ap.parse_args()

    import numpy as np
    import torch

    import vectorwave_amd as vw
    from vectorwave_amd import _native as nat

    if not torch.cuda.is_available():
        print("energybench needs a GPU (no fallback)", file=sys.stderr)
        return 1
    B, N, J = args.batch, args.length, args.levels
    w = vw.Daubechies.DB4
    lo, hi = w.lowPassDecomposition(), w.highPassDecomposition()
    tlo, thi = nat.taps_array(lo), nat.taps_array(hi)
    eng = vw.Engine.get(0)
    in_bytes = B * N * 8
    sets = max(2, -(-(512 << 20) // in_bytes))
    xs = [eng.fill_uniform(torch.empty((B, N), dtype=torch.float64, device="cuda"), 42 + i) for i in range(sets)]
    outs = [torch.empty((J + 1, B), dtype=torch.float64, device="cuda") for _ in range(sets)]
    eng.bind_torch_stream()

    def energy(flags):
        def step(i):
            x, out = xs[i % sets], outs[i % sets]
            st = eng.lib.vw_modwt_energy_f64(eng.ctx, c_void_p(x.data_ptr()), B, N, N, tlo, thi, len(lo), w.wavelet_id,
                                             0, J, flags, c_void_p(out.data_ptr()))
            assert st == 0, nat.last_error()
            return out
        return step

    def composed(i):
        det, app = eng.forward(xs[i % sets], lo, hi, w.wavelet_id, 0, J, 0)
        return torch.cat([(app * app).sum(-1)[None], (det * det).sum(-1)])

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

    # the computations agree before anything is timed
    ex, tr, co = energy(0)(0).clone(), energy(nat.FLAG_TREE_SUMS)(0).clone(), composed(0)
    torch.cuda.synchronize()
    for got in (tr, co):
        assert torch.allclose(got, ex, rtol=N * 2.0 ** -52, atol=0.0), ((got - ex).abs() / ex).max()

    # kernel times of the two engine paths (HIP events around each launch)
    eng.enable_timing(True)
    eng.reset_timing()
    energy(0)(1)
    energy(nat.FLAG_TREE_SUMS)(1)
    eng.synchronize()
    kern = {fam: round(eng.kernel_time(fam)[0] * 1e3, 2) for fam in ("forward", "energy_chain", "energy_fused")}
    eng.enable_timing(False)
    eng.reset_timing()

    res = {"shape": [B, N], "levels": J, "sets": sets, "steps": args.steps, "input_mb": in_bytes / 1e6,
           "kernel_us": kern}
    for name, step in (("exact", energy(0)), ("tree", energy(nat.FLAG_TREE_SUMS)), ("composed", composed),
                       ("read", read)):
        res[name + "_us"] = round(time_us(step), 2)

    # the host path: device-to-host copy of all planes, then the sequential numpy pass per plane
    det, app = eng.forward(xs[0], lo, hi, w.wavelet_id, 0, J, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dh, ah = det.cpu().numpy(), app.cpu().numpy()
    t1 = time.perf_counter()
    rows = min(B, args.host_rows)
    planes = np.concatenate([ah[None, :rows], dh[:, :rows]])
    host_e = np.add.accumulate(planes * planes, axis=-1)[..., -1]
    t2 = time.perf_counter()
    assert np.array_equal(host_e, ex[:, :rows].cpu().numpy()), "exact mode is not the host path's bits"
    res["host_copy_ms"] = round((t1 - t0) * 1e3, 1)
    res["host_sum_ms"] = round((t2 - t1) * 1e3 * B / rows, 1)
    res["host_ms"] = round(res["host_copy_ms"] + res["host_sum_ms"], 1)

    plane_bytes = (J + 1) * B * N * 8
    res["bytes_mb"] = {"tree": round((in_bytes + (J + 1) * B * 8) / 1e6, 1),
                       "composed": round((in_bytes + 2 * plane_bytes) / 1e6, 1),
                       "exact": round((in_bytes + 2 * plane_bytes) / 1e6, 1)}
    res["read_gbps"] = round(in_bytes / res["read_us"] / 1e3, 1)
    res["tree_over_read"] = round(res["tree_us"] / res["read_us"], 2)
    res["composed_over_tree"] = round(res["composed_us"] / res["tree_us"], 2)
    res["host_over_exact"] = round(res["host_ms"] * 1e3 / res["exact_us"], 1)
    for k in ("exact", "tree", "composed", "read"):
        print(f"{k:9s} {res[k + '_us']:10.1f} us")
    print(f"{'host':9s} {res['host_ms']:10.1f} ms (copy {res['host_copy_ms']}, sums {res['host_sum_ms']})")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
