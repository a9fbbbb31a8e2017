"""Child process of tests/test_subgraph_softmax_gpu.py::test_device_tensors_autograd_and_attention: Engine.subgraph_softmax and
_bwd over device tensors read and written in place, torch_ops.subgraph_edge_softmax with its backward pass, and
torch_ops.subgraph_attention against the composition of the three twins.  torch is imported first, so that the library binds
to the HIP runtime torch brought along."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import subgraph_prop_ref as sr  # noqa: E402
import subgraph_ref  # noqa: E402
import subgraph_sddmm_ref as ss  # noqa: E402
import subgraph_softmax_ref as sm  # noqa: E402
import fora_amd  # noqa: E402
from fora_amd import torch_ops  # noqa: E402
from subgraph_prop_device_child import same  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    engine = fora_amd.Engine(0)
    row_ptr_g, col, U = sr.crafted_graph()
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(row_ptr_g, col, U)
    nc, edges, d, heads = U.size, sub_col.size, 8, 2
    engine.set_graph(sr.CRAFTED_N, int(row_ptr_g[-1]), row_ptr_g, col)
    engine.store_load(np.array([0, nc], dtype=np.int64), U, np.full(nc, 1 << 40, dtype=np.uint64))
    engine.set_option("softmax_short", 64)                                      # both paths in every call
    engine.store_take_subgraph([0, 0])
    rng = np.random.Generator(np.random.PCG64(9990))
    dn = lambda x: torch.from_numpy(x).to(dev)
    s = (rng.standard_normal((heads, edges)) * 4.0).astype(np.float32)
    g = rng.standard_normal((heads, edges)).astype(np.float32)

    for by in ("row", "col"):
        y64, y32, _ = sm.forward(sub_ptr, sub_col, s, 0.5, by)
        dx64, dx32 = sm.backward(sub_ptr, sub_col, y32, g, 0.5, by)
        # ---- device tensors in and out in place: a slice of a wider tensor, a caller-made output, one operand on the host
        wide = torch.zeros((heads + 1, edges), device=dev)
        wide[1:] = dn(s)
        o32, o64, st = engine.subgraph_softmax(wide[1:], scale=0.5, by=by, want64=True)
        assert o32.is_cuda and o64.is_cuda and st["nan_groups"] == 0 and st["long_groups"] == 6
        same(o32, y32, f"y32 {by}")
        same(o64, y64, f"y64 {by}")
        buf = torch.full((heads, edges), 7.0, dtype=torch.float64, device=dev)
        engine.subgraph_softmax_bwd(o32, g, scale=0.5, by=by, want32=False, out64=buf)
        same(buf, dx64, f"a caller-made dx64 {by}")
        # ---- torch_ops.subgraph_edge_softmax: forward and backward are the twins' bits, the gradient in the leaf's dtype
        for dtype in (torch.float32, torch.float64):
            leaf = dn(s).to(dtype).requires_grad_(True)
            y = torch_ops.subgraph_edge_softmax(engine, leaf, scale=0.5, by=by)
            same(y, y32, f"forward {by} {dtype}")
            y.backward(dn(g))
            same(leaf.grad, dx32 if dtype == torch.float32 else dx32.astype(np.float64), f"scores.grad {by} {dtype}")

    # ---- torch_ops.subgraph_attention: the composition of the three twins in both directions; V.grad is the opposite product
    Q, K, V, G = (rng.standard_normal((nc, heads * d)).astype(np.float32) for _ in range(4))
    for direction, by, ab, fwd, back in (("out", "row", (Q, K), sr.propagate, sr.propagate_t), ("in", "col", (K, Q), sr.propagate_t, sr.propagate)):
        y32 = sm.forward(sub_ptr, sub_col, ss.scores(sub_ptr, sub_col, *ab, heads=heads)[1], d ** -0.5, by)[1]
        Ql, Kl, Vl = (dn(x).requires_grad_(True) for x in (Q, K, V))
        out = torch_ops.subgraph_attention(engine, Ql, Kl, Vl, heads=heads, direction=direction)
        out.backward(dn(G))
        for h in range(heads):
            cs = slice(h * d, (h + 1) * d)
            same(out[:, cs].contiguous(), fwd(sub_ptr, sub_col, np.ascontiguousarray(V[:, cs]), values=y32[h])[1], f"attention {direction} head {h}")
            same(Vl.grad[:, cs].contiguous(), back(sub_ptr, sub_col, np.ascontiguousarray(G[:, cs]), values=y32[h])[1], f"V.grad {direction} head {h}")
        assert torch.isfinite(Ql.grad).all() and torch.isfinite(Kl.grad).all() and Ql.grad.abs().sum() > 0 and Kl.grad.abs().sum() > 0

    # ---- the generation guard
    loss = torch_ops.subgraph_edge_softmax(engine, dn(s).requires_grad_(True)).sum()
    engine.store_take_subgraph([0, 0])                                          # the held result was replaced (by an equal one)
    try:
        loss.backward()
        raise AssertionError("a backward pass after the held result was replaced went through")
    except RuntimeError as e:
        assert "replaced or cleared" in str(e)
    engine.close()
    print("subgraph softmax device ok")


if __name__ == "__main__":
    main()
