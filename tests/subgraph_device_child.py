"""Child process of tests/test_subgraph_gpu.py::test_device_tensors_and_edge_index: Engine.store_take_subgraph with device
tensors, and capi.subgraph_edge_index over them.  torch is imported first, so that the library binds to the HIP runtime torch
brought along and a tensor's data_ptr() is device memory the library knows."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import subgraph_ref  # noqa: E402
import fora_amd  # noqa: E402
from fora_amd import capi, synth  # noqa: E402
from test_sparse_gpu import SEED  # noqa: E402


def main():
    assert torch.cuda.is_available()
    engine = fora_amd.Engine(0)
    n, m, row_ptr_g, col = synth.preset("tiny", "rmat")
    engine.set_graph(n, m, row_ptr_g, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    rng = np.random.Generator(np.random.PCG64(9800))
    pool = rng.choice(np.flatnonzero(np.diff(row_ptr_g) > 0), 9, replace=False).astype(np.int32)
    pick = np.array([4, 4, 8, 0, 2, 6], dtype=np.int64)
    engine.store_put(engine.query_sparse_topk(pool, 16, threshold=0.0)[0])

    row_ptr, cols, sub_ptr, sub_col, sub_eid, st = engine.store_take_subgraph(pick, want_eid=True, device=True)
    want = subgraph_ref.induced(row_ptr_g, col, cols.cpu().numpy())
    for t, dtype, w in zip((sub_ptr, sub_col, sub_eid), (torch.int64, torch.int32, torch.int64), want):
        assert t.is_cuda and t.device.index == engine.device and t.dtype == dtype and t.shape == w.shape
        assert (t.cpu().numpy() == w).all()
    assert st["edges"] == want[1].size > 0 and st["scanned"] == want[3]
    # the same build into host arrays; without the edge ids
    h = engine.sparse_subgraph(row_ptr, want_eid=True)
    assert all((a == w).all() for a, w in zip(h[:3], want))
    assert engine.sparse_subgraph(row_ptr, device=True)[2] is None

    # the COO pair, on the device and on the host
    ei = capi.subgraph_edge_index(sub_ptr, sub_col)
    assert ei.is_cuda and ei.dtype == torch.int64 and ei.shape == (2, st["edges"])
    ei_host = capi.subgraph_edge_index(h[0], h[1])
    assert (ei.cpu().numpy() == ei_host).all()
    src, dst = ei_host
    local = cols.cpu().numpy()
    assert (col[h[2]] == local[dst]).all()                                     # the edge sub_eid names ends at the target's node
    assert all(row_ptr_g[local[s]] <= e < row_ptr_g[local[s] + 1] for s, e in zip(src, h[2]))  # ... and starts at the source's
    engine.close()
    print("subgraph device ok")


if __name__ == "__main__":
    main()
