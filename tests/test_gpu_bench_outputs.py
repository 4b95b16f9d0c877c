"""bench.py --dump-outputs on the GPU: the arrays written are the last timed step's results.

A 64 x 4096 db4 batch in EXACT accumulation, so every dumped row must equal the restatement of
vectorwave-core bit for bit (the bench's input is the counter-based generator, seed 42, which the oracle
restates).  Both step schedules of the fwd+inv pipeline: consecutive steps overlapped on two contexts (the
policy at 64 rows; the last set comes from the engine's pipeline) and the rows split over two contexts (as
the headline's four; the dump joins the contexts' blocks).  Three steps over two rotated buffer sets, so
the last step's set is not set 0's neighbour by accident of a single step.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from vectorwave_amd.wavelets import Daubechies

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, J = 64, 4096, 6


@pytest.fixture(scope="module")
def expected():
    w = Daubechies.DB4
    x = O.fill_uniform(B * N, 42).reshape(B, N)
    out = {}
    for b in (0, 31, 32, B - 1):   # both ends of both contexts' blocks
        # core=False: the batch semantics of the bench's C-ABI calls (no VW_FLAG_CORE_LEVELS), as bench.verify
        d, a = O.decompose(x[b], w.lowPassDecomposition(), w.highPassDecomposition(), O.PERIODIC, J, core=False)
        y = O.reconstruct(d, a, w.lowPassReconstruction(), w.highPassReconstruction(), O.PERIODIC, w.wavelet_id)
        out[b] = (d, a, y)
    return out


@pytest.mark.parametrize("schedule", [[], ["--contexts", "2"]], ids=["overlap-steps", "contexts"])
def test_dump_outputs_are_the_last_steps_results(engine, expected, tmp_path, schedule):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--settle", "0", "--batch", str(B), "--exact", "--dump-outputs", str(tmp_path), *schedule],
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and not line["full"]
    assert line["config"]["schedule"] == ("contexts" if schedule else "overlap-steps")
    assert line["outputs"]["rows"] == list(range(B)) and line["outputs"]["columns"] == "all"
    assert sorted(os.listdir(tmp_path)) == ["app.npy", "det.npy", "y.npy"]
    det, app, y = (np.load(tmp_path / f"{k}.npy") for k in ("det", "app", "y"))
    assert det.shape == (J, B, N) and app.shape == (B, N) and y.shape == (B, N)
    assert det.dtype == app.dtype == y.dtype == np.float64
    for b, (d_ref, a_ref, y_ref) in expected.items():
        assert np.array_equal(det[:, b, :], d_ref), f"details row {b}"
        assert np.array_equal(app[b], a_ref), f"approximation row {b}"
        assert np.array_equal(y[b], y_ref), f"reconstruction row {b}"
