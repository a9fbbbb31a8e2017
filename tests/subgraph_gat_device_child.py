"""Child process of tests/test_subgraph_gat_gpu.py::test_device_tensors_and_autograd: Engine.subgraph_gat over device tensors read
in place with a pitched caller-made output, and torch_ops.subgraph_gat -- forward against the twin's out32, el.grad, er.grad and
V.grad bit for bit against the backward twin on the saved y32, in both directions.  torch is imported first, so that the library
binds to the HIP runtime torch brought along."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import subgraph_gat_ref as gat  # noqa: E402
import subgraph_prop_ref as sr  # noqa: E402
import subgraph_ref  # noqa: E402
import fora_amd  # noqa: E402
from fora_amd import torch_ops  # noqa: E402
from subgraph_prop_device_child import same  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    engine = fora_amd.Engine(0)
    row_ptr_g, col, U = sr.crafted_graph()
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(row_ptr_g, col, U)
    nc, dv, heads = U.size, 8, 2
    engine.set_graph(sr.CRAFTED_N, int(row_ptr_g[-1]), row_ptr_g, col)
    engine.store_load(np.array([0, nc], dtype=np.int64), U, np.full(nc, 1 << 40, dtype=np.uint64))
    engine.set_option("attn_short", 64)                                         # both paths in every call
    engine.store_take_subgraph([0, 0])
    rng = np.random.Generator(np.random.PCG64(10600))
    dn = lambda x: torch.from_numpy(x).to(dev)
    el, er, V, G = (rng.standard_normal((nc, w)).astype(np.float32) for w in (heads, heads, heads * dv, heads * dv))
    for direction, by in (("out", "row"), ("in", "col")):
        out64, out32, _, y32, _ = gat.forward(sub_ptr, sub_col, el, er, V, heads=heads, slope=0.2, by=by)
        want = gat.backward(sub_ptr, sub_col, el, er, V, G, y32, heads=heads, slope=0.2, by=by)
        # ---- device tensors in place: column slices of a wider tensor, a caller-made out64 with a pitch
        wide = torch.zeros((nc, 2 * heads + heads * dv + 4), device=dev)
        views = [wide[:, 1:1 + heads], wide[:, 2 + heads:2 + 2 * heads], wide[:, 3 + 2 * heads:3 + 2 * heads + heads * dv]]
        for view, x in zip(views, (el, er, V)):
            view.copy_(dn(x))
        buf = torch.full((nc, heads * dv + 3), 7.0, dtype=torch.float64, device=dev)
        _, _, y, _, st = engine.subgraph_gat(*views, heads=heads, by=by, want32=False, out64=buf[:, :heads * dv], want_y32=True)
        assert y.is_cuda and st["long_groups"] == 6 and (buf[:, heads * dv:] == 7.0).all()
        same(buf[:, :heads * dv].contiguous(), out64, f"a caller-made out64 {by}")
        same(y, y32, f"y32 {by}")
        # ---- torch_ops.subgraph_gat: the twin's out32, and the backward twin's gradients on the saved y32
        leaves = [dn(x).requires_grad_(True) for x in (el, er, V)]
        out = torch_ops.subgraph_gat(engine, *leaves, heads=heads, direction=direction)
        same(out, out32, f"forward {direction}")
        out.backward(dn(G))
        for leaf, w, name in zip(leaves, want[1::2], ("el.grad", "er.grad", "V.grad")):
            same(leaf.grad, w, f"{name} {direction}")
        assert (engine.last_subgraph_gat_bwd["long_groups"], engine.last_subgraph_gat_bwd["across_long"]) == (6, 6)
    # ---- the generation guard
    loss = torch_ops.subgraph_gat(engine, dn(el).requires_grad_(True), dn(er), dn(V), heads=heads).sum()
    engine.store_take_subgraph([0, 0])                                          # the held result was replaced (by an equal one)
    try:
        loss.backward()
        raise AssertionError("a backward pass after the held result was replaced went through")
    except RuntimeError as e:
        assert "replaced or cleared" in str(e)
    engine.close()
    print("subgraph gat device ok")


if __name__ == "__main__":
    main()
