"""Child process of tests/test_sweep_gpu.py::test_device_fetch: Engine.sweep(device=True) and Engine.sweep_fetch into torch
tensors.  torch is imported first, so that the library binds to the HIP runtime torch brought along and a tensor's
data_ptr() is device memory the library knows."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fora_amd  # noqa: E402
from fora_amd import synth  # noqa: E402
from test_sweep_gpu import G, SEED, check  # noqa: E402


def main():
    assert torch.cuda.is_available()
    engine = fora_amd.Engine(0)
    n, m, row_ptr, col = synth.preset("tiny", "rmat")
    g = G(n, row_ptr, col)
    rng = np.random.Generator(np.random.PCG64(8800))
    live = rng.choice(np.flatnonzero(g.deg > 0), 4, replace=False)
    dang = rng.choice(np.flatnonzero(g.deg == 0), 1)
    srcs = np.concatenate([live[:2], dang, live[2:]]).astype(np.int32)
    engine.set_graph(n, m, g.row_ptr, g.col)
    engine.set_params(epsilon=0.5, seed=SEED)
    want, _, wst = engine.query_fix(srcs)
    for t, max_size in ((None, 0), (0.0, 500)):
        dev = engine.sweep(srcs, threshold=t, max_size=max_size, want_profile=True, device=True)
        for x, dt in ((dev["ids"], torch.int32), (dev["cut"], torch.int64), (dev["vol"], torch.int64)):
            assert x.is_cuda and x.device.index == engine.device and x.dtype == dt
        e = int(dev["row_ptr"][-1])
        ids, cut, vol = engine.sweep_fetch(e)   # the held result again, into host arrays
        assert (dev["ids"].cpu().numpy() == ids).all()
        assert (dev["cut"].cpu().numpy().view(np.uint64) == cut).all() and (dev["vol"].cpu().numpy().view(np.uint64) == vol).all()
        host = dict(dev, ids=ids, cut=cut, vol=vol)
        check(g, want, wst, t, max_size, host)
    engine.close()
    print("sweep device ok")


if __name__ == "__main__":
    main()
