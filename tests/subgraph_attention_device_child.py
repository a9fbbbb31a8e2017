"""Child process of tests/test_subgraph_attention_gpu.py::test_device_tensors_and_autograd: Engine.subgraph_attention over device
tensors read and written in place, and torch_ops.subgraph_attention_fused -- forward against the twin's out32, Q.grad, K.grad and
V.grad bit for bit against the chain of twins on the saved y32 (every step of the backward pass is a defined call).  torch is
imported first, so that the library binds to the HIP runtime torch brought along."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import subgraph_attention_ref as at  # noqa: E402
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
    nc, d, heads = U.size, 8, 2
    engine.set_graph(sr.CRAFTED_N, int(row_ptr_g[-1]), row_ptr_g, col)
    engine.store_load(np.array([0, nc], dtype=np.int64), U, np.full(nc, 1 << 40, dtype=np.uint64))
    engine.set_option("attn_short", 64)                                         # both paths in every call
    engine.store_take_subgraph([0, 0])
    rng = np.random.Generator(np.random.PCG64(10200))
    dn = lambda x: torch.from_numpy(x).to(dev)
    Q, K, V, G = (rng.standard_normal((nc, heads * d)).astype(np.float32) for _ in range(4))
    scale = d ** -0.5
    for direction, by, along, across in (("out", "row", sr.propagate, sr.propagate_t), ("in", "col", sr.propagate_t, sr.propagate)):
        out64, out32, y64, y32, _ = at.attention(sub_ptr, sub_col, Q, K, V, heads=heads, scale=scale, by=by)
        # ---- device tensors in and out in place: column slices of a wider tensor, a caller-made output with a pitch
        wide = torch.zeros((nc, 3 * heads * d + 5), device=dev)
        views = [wide[:, 1 + i * heads * d:1 + (i + 1) * heads * d] for i in range(3)]
        for view, x in zip(views, (Q, K, V)):
            view.copy_(dn(x))
        buf = torch.full((nc, heads * d + 3), 7.0, dtype=torch.float64, device=dev)
        _, _, a32, a64, st = engine.subgraph_attention(*views, heads=heads, by=by, want32=False, want_y32=True, want_y64=True, out64=buf[:, :heads * d])
        assert a32.is_cuda and a64.is_cuda and (st["long_groups"], st["nan_pairs"]) == (6, 0) and (buf[:, heads * d:] == 7.0).all()
        for got, want, name in ((buf[:, :heads * d].contiguous(), out64, "a caller-made out64"), (a32, y32, "y32"), (a64, y64, "y64")):
            same(got, want, f"{name} {by}")
        # ---- torch_ops.subgraph_attention_fused: the twin's out32, and the gradients of the chain of twins on the saved y32
        Ql, Kl, Vl = (dn(x).requires_grad_(True) for x in (Q, K, V))
        out = torch_ops.subgraph_attention_fused(engine, Ql, Kl, Vl, heads=heads, direction=direction)
        same(out, out32, f"forward {direction}")
        out.backward(dn(G))
        dy = ss.scores(sub_ptr, sub_col, *((G, V) if by == "row" else (V, G)), heads=heads)[1]
        ds = sm.backward(sub_ptr, sub_col, y32, dy, scale, by)[1]
        for h in range(heads):
            cs, part = slice(h * d, (h + 1) * d), lambda X: np.ascontiguousarray(X[:, h * d:(h + 1) * d])
            same(Vl.grad[:, cs].contiguous(), across(sub_ptr, sub_col, part(G), values=y32[h])[1], f"V.grad {direction} head {h}")
            same(Ql.grad[:, cs].contiguous(), along(sub_ptr, sub_col, part(K), values=ds[h])[1], f"Q.grad {direction} head {h}")
            same(Kl.grad[:, cs].contiguous(), across(sub_ptr, sub_col, part(Q), values=ds[h])[1], f"K.grad {direction} head {h}")

    # ---- the generation guard
    loss = torch_ops.subgraph_attention_fused(engine, dn(Q).requires_grad_(True), dn(K), dn(V), heads=heads).sum()
    engine.store_take_subgraph([0, 0])                                          # the held result was replaced (by an equal one)
    try:
        loss.backward()
        raise AssertionError("a backward pass after the held result was replaced went through")
    except RuntimeError as e:
        assert "replaced or cleared" in str(e)
    engine.close()
    print("subgraph attention device ok")


if __name__ == "__main__":
    main()
