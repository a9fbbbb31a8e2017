"""Child process of tests/test_subgraph_attention_bwd_gpu.py::test_device_tensors_and_autograd: Engine.subgraph_attention_bwd over
device tensors read and written in place, and torch_ops.subgraph_attention_trained -- forward against the twin's out32, Q.grad,
K.grad and V.grad bit for bit against the backward twin on the saved y32.  torch is imported first, so that the library binds to
the HIP runtime torch brought along."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import subgraph_attention_bwd_ref as bw  # noqa: E402
import subgraph_attention_ref as at  # noqa: E402
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
    nc, d, heads = U.size, 8, 2
    engine.set_graph(sr.CRAFTED_N, int(row_ptr_g[-1]), row_ptr_g, col)
    engine.store_load(np.array([0, nc], dtype=np.int64), U, np.full(nc, 1 << 40, dtype=np.uint64))
    engine.set_option("attn_short", 64)                                         # both paths in every call
    engine.store_take_subgraph([0, 0])
    rng = np.random.Generator(np.random.PCG64(10400))
    dn = lambda x: torch.from_numpy(x).to(dev)
    Q, K, V, G = (rng.standard_normal((nc, heads * d)).astype(np.float32) for _ in range(4))
    scale = d ** -0.5
    for direction, by in (("out", "row"), ("in", "col")):
        _, out32, _, y32, _ = at.attention(sub_ptr, sub_col, Q, K, V, heads=heads, scale=scale, by=by)
        want = bw.backward(sub_ptr, sub_col, Q, K, V, G, y32, heads=heads, scale=scale, by=by)
        # ---- device tensors in place: column slices of a wider tensor, a caller-made dk64 with a pitch
        wide = torch.zeros((nc, 4 * heads * d + 5), device=dev)
        views = [wide[:, 1 + i * heads * d:1 + (i + 1) * heads * d] for i in range(4)]
        for view, x in zip(views, (Q, K, V, G)):
            view.copy_(dn(x))
        buf = torch.full((nc, heads * d + 3), 7.0, dtype=torch.float64, device=dev)
        _, dq64, _, _, _, dv64, st = engine.subgraph_attention_bwd(*views, dn(y32), heads=heads, by=by, want32=False, want64=True, dk64=buf[:, :heads * d])
        assert dq64.is_cuda and dv64.is_cuda and (st["long_groups"], st["across_long"]) == (6, 6) and (buf[:, heads * d:] == 7.0).all()
        for got, w, name in ((dq64, want[0], "dq64"), (buf[:, :heads * d].contiguous(), want[2], "a caller-made dk64"), (dv64, want[4], "dv64")):
            same(got, w, f"{name} {by}")
        # ---- torch_ops.subgraph_attention_trained: the twin's out32, and the backward twin's gradients on the saved y32
        Ql, Kl, Vl = (dn(x).requires_grad_(True) for x in (Q, K, V))
        out = torch_ops.subgraph_attention_trained(engine, Ql, Kl, Vl, heads=heads, direction=direction)
        same(out, out32, f"forward {direction}")
        out.backward(dn(G))
        for leaf, w, name in ((Ql, want[1], "Q.grad"), (Kl, want[3], "K.grad"), (Vl, want[5], "V.grad")):
            same(leaf.grad, w, f"{name} {direction}")
        # ---- only Q requires grad: dk and dv are absent, the across side does not run
        Ql = dn(Q).requires_grad_(True)
        torch_ops.subgraph_attention_trained(engine, Ql, dn(K), dn(V), heads=heads, direction=direction).backward(dn(G))
        same(Ql.grad, want[1], f"Q.grad alone {direction}")
        assert (engine.last_subgraph_attention_bwd["across_short"], engine.last_subgraph_attention_bwd["across_long"]) == (0, 0)

    # ---- the generation guard
    loss = torch_ops.subgraph_attention_trained(engine, dn(Q).requires_grad_(True), dn(K), dn(V), heads=heads).sum()
    engine.store_take_subgraph([0, 0])                                          # the held result was replaced (by an equal one)
    try:
        loss.backward()
        raise AssertionError("a backward pass after the held result was replaced went through")
    except RuntimeError as e:
        assert "replaced or cleared" in str(e)
    engine.close()
    print("subgraph attention bwd device ok")


if __name__ == "__main__":
    main()
