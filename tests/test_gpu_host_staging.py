"""Host-memory calls (VW_FLAG_HOST_MEMORY: staged in, run, staged out) give the bits of the device-pointer call on
the same input, for every entry point that takes the flag: both run the same kernels on the same values, so there
is no tolerance.  Row inputs are exactly (B - 1) * ld + N elements long with ld = N + 8: the last row's padding
does not exist."""
import numpy as np
import pytest

import host_calls as H
from vectorwave_amd import _native as nat

pytestmark = pytest.mark.gpu

B, N, J = 3, 48, 2
CASES = [(name, nat.PERIODIC) for name in sorted(H.CALLS)] + [("vw_modwt1_forward_f64", nat.SYMMETRIC),
                                                                ("vw_swt_denoise_f64", nat.SYMMETRIC)]


@pytest.mark.parametrize("name,boundary", CASES, ids=[f"{n}-{'periodic' if b == nat.PERIODIC else 'symmetric'}"
                                                      for n, b in CASES])
def test_host_memory_call_matches_device_call(engine, name, boundary):
    import torch
    engine.bind_torch_stream()
    lib, ctx = engine.lib, engine.ctx
    got = []
    for side in (H.Side(), H.Side(torch)):
        assert H.CALLS[name](lib, ctx, side, B, N, J, boundary) == 0, nat.last_error()
        got.append(side.results())
        side.close(lib)
    host, dev = got
    assert len(host) == len(dev) >= 1
    for h, d in zip(host, dev):
        assert h.dtype == d.dtype and h.shape == d.shape
        assert not np.isnan(d).any()  # (every output element was written)
        assert np.array_equal(h, d)
