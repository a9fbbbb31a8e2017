"""Child process of tests/test_cols_gpu.py::test_device_tensors_and_autograd: Engine.store_take_compact with a device tensor of
columns, and the torch_ops functions over X[cols].  torch is imported first, so that the library binds to the HIP runtime torch
brought along and a tensor's data_ptr() is device memory the library knows."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cols_ref  # noqa: E402
import fora_amd  # noqa: E402
from fora_amd import synth, torch_ops  # noqa: E402
from test_sparse_gpu import SEED  # noqa: E402


def main():
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    engine = fora_amd.Engine(0)
    n, m, row_ptr_g, col = synth.preset("tiny", "rmat")
    engine.set_graph(n, m, row_ptr_g, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    deg = np.diff(row_ptr_g)
    rng = np.random.Generator(np.random.PCG64(9600))
    pool = rng.choice(np.flatnonzero(deg > 0), 9, replace=False).astype(np.int32)
    pick = np.array([4, 4, 8, 0, 2, 6], dtype=np.int64)
    heads, d, dv, K_TOP = 2, 8, 6, 16
    engine.store_put(engine.query_sparse_topk(pool, K_TOP, threshold=0.0)[0])

    # ---- the columns as a device tensor are the twin's
    row_ptr, _ = engine.store_take(pick)
    e = int(row_ptr[-1])
    ids = np.zeros(e, np.int32)
    engine.sparse_fetch(ids, None, None, cap=e)
    want_cols, want_local = cols_ref.compact(ids)
    rp2, cols, st = engine.store_take_compact(pick, device=True)
    assert (rp2 == row_ptr).all() and st["cols"] == want_cols.size and st["entries"] == e
    assert cols.is_cuda and cols.dtype == torch.int32 and cols.shape == (want_cols.size,)
    assert (cols.cpu().numpy() == want_cols).all()
    engine.sparse_fetch(ids, None, None, cap=e)
    assert (ids == want_local).all() and engine.held_cols == want_cols.size < n

    # ---- autograd over X[cols]: the outputs and the gradients with respect to X of the uncompacted run
    gen = torch.Generator(device="cpu").manual_seed(9601)
    Q0 = torch.randn(len(pick), heads * d, generator=gen).to(dev)
    K0 = torch.randn(n, heads * d, generator=gen).to(dev)
    V0 = torch.randn(n, heads * dv, generator=gen).to(dev)
    W = torch.randn(len(pick), heads * dv, generator=gen).to(dev)

    def grads(row_ptr, index):
        Q, K, V = (x.clone().requires_grad_(True) for x in (Q0, K0, V0))
        Kx, Vx = (K, V) if index is None else (K[index], V[index])
        out = torch_ops.ppr_attention_fused(engine, row_ptr, Q, Kx, Vx, heads=heads, backward="fused")
        (out * W).sum().backward()
        return out.detach(), Q.grad, K.grad, V.grad

    row_ptr, _ = engine.store_take(pick)
    full = grads(row_ptr, None)
    row_ptr, cols, _ = engine.store_take_compact(pick, device=True)
    local = grads(row_ptr, cols.long())
    for a, b in zip(full, local):
        assert a.shape == b.shape and torch.equal(a, b)
    assert float(local[2].abs().sum()) > 0 and float(local[3].abs().sum()) > 0

    # ---- a compaction between forward and backward is refused by the guard
    row_ptr, _ = engine.store_take(pick)
    Q = Q0.clone().requires_grad_(True)
    out = torch_ops.ppr_attention_fused(engine, row_ptr, Q, K0, V0, heads=heads, backward="fused")
    engine.sparse_compact(row_ptr)
    try:
        out.sum().backward()
        raise AssertionError("the backward pass ran on rows that were compacted after the forward pass")
    except RuntimeError as err:
        assert "replaced or cleared" in str(err)
    engine.close()
    print("cols device ok")


if __name__ == "__main__":
    main()
