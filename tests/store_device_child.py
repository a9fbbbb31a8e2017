"""Child process of tests/test_store_gpu.py::test_device_arrays_and_autograd: Engine.store_load from torch device tensors, and
the torch_ops functions on a row_ptr that Engine.store_take returned.  torch is imported first, so that the library binds to
the HIP runtime torch brought along and a tensor's data_ptr() is device memory the library knows."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fora_amd  # noqa: E402
import store_ref  # noqa: E402
from fora_amd import synth, torch_ops  # noqa: E402
from test_sparse_gpu import SEED  # noqa: E402
from test_store_gpu import _crafted, _same, _take, _twin  # noqa: E402


def main():
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    engine = fora_amd.Engine(0)
    n, m, row_ptr_g, col = synth.preset("tiny", "rmat")
    engine.set_graph(n, m, row_ptr_g, col)
    engine.set_params(epsilon=0.5, seed=SEED)

    # ---- store_load from device tensors gives the host load's bits
    store = _crafted(n, seed=8800)
    R, e = len(store[0]) - 1, int(store[0][-1])
    rows = np.random.Generator(np.random.PCG64(8801)).permutation(R)
    engine.store_load(*store)
    want = _take(engine, rows)
    _same(want, _twin(store, rows))
    big = torch.full((e + 3,), -7, dtype=torch.int32, device=dev)
    big[3:] = torch.from_numpy(store[1]).to(dev)
    ids_t = big[3:]                                   # an offset slice of a larger tensor: 4-byte aligned, not 16
    assert ids_t.data_ptr() % 16 == 12
    fix_t = torch.from_numpy(store[2].view(np.int64)).to(dev)
    for ids, fix, flags in ((ids_t, fix_t, (1, 1)), (store[1], fix_t, (0, 1)), (ids_t, store[2], (1, 0))):
        engine.store_clear()
        st = engine.store_load(store[0], ids, fix)
        assert (st["ids_on_device"], st["fix_on_device"]) == flags and st["store_entries"] == e
        _same(_take(engine, rows), want)
    # ... by two appends, and a bad device array is refused with the store left alone
    cut = 7
    c = int(store[0][cut])
    engine.store_load(store[0][:cut + 1], ids_t[:c], fix_t[:c])
    engine.store_load(store[0][cut:] - c, ids_t[c:], fix_t[c:], append=True)
    _same(_take(engine, rows), want)
    bad = ids_t.clone()
    k = int(store[0][5]) + 1                          # the second entry of the row of 65: made equal to the first
    bad[k] = bad[k - 1]
    assert store_ref.first_bad_entry(store[0], bad.cpu().numpy(), n) == k
    try:
        engine.store_load(store[0], bad, fix_t)
        raise AssertionError("a bad device array was accepted")
    except fora_amd.ForaError as err:
        assert err.code == -1 and f"entry {k} " in str(err)
    _same(_take(engine, rows), want)

    # ---- autograd on a taken row_ptr: the gradients of the same call on a directly queried result
    deg = np.diff(row_ptr_g)
    rng = np.random.Generator(np.random.PCG64(8802))
    pool = rng.choice(np.flatnonzero(deg > 0), 9, replace=False).astype(np.int32)
    pick = np.array([4, 4, 8, 0, 2, 6], dtype=np.int64)
    heads, d, dv, K_TOP = 2, 8, 6, 64
    gen = torch.Generator(device="cpu").manual_seed(8803)
    Q0 = torch.randn(len(pick), heads * d, generator=gen).to(dev)
    K0 = torch.randn(n, heads * d, generator=gen).to(dev)
    V0 = torch.randn(n, heads * dv, generator=gen).to(dev)
    W = torch.randn(len(pick), heads * dv, generator=gen).to(dev)

    def grads(row_ptr):
        Q, K, V = (x.clone().requires_grad_(True) for x in (Q0, K0, V0))
        out = torch_ops.ppr_attention_fused(engine, row_ptr, Q, K, V, heads=heads, backward="fused")
        (out * W).sum().backward()
        return out.detach(), Q.grad, K.grad, V.grad

    direct = grads(engine.query_sparse_topk(pool[pick], K_TOP, threshold=0.0)[0])
    engine.store_put(engine.query_sparse_topk(pool, K_TOP, threshold=0.0)[0])
    row_ptr, _ = engine.store_take(pick)
    taken = grads(row_ptr)
    for a, b in zip(direct, taken):
        assert a.shape == b.shape and torch.equal(a, b)
    assert float(taken[2].abs().sum()) > 0

    # ---- a backward pass after a later take is refused by the guard
    Q = Q0.clone().requires_grad_(True)
    out = torch_ops.ppr_attention_fused(engine, row_ptr, Q, K0, V0, heads=heads, backward="fused")
    engine.store_take(pick)
    try:
        out.sum().backward()
        raise AssertionError("the backward pass ran on rows that were taken again")
    except RuntimeError as err:
        assert "replaced or cleared" in str(err)
    engine.close()
    print("store device ok")


if __name__ == "__main__":
    main()
