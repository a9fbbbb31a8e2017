"""Child process of tests/test_subgraph_gatv2_gpu.py::test_device_tensors_and_autograd: device tensors read in place, and
torch_ops.subgraph_gatv2 against the twin and float64 autograd.  torch is imported first: one HIP runtime in the process."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import subgraph_gatv2_ref as g2  # noqa: E402
import subgraph_prop_ref as sr  # noqa: E402
import subgraph_ref  # noqa: E402
from subgraph_prop_device_child import same  # noqa: E402

HEADS, D, DV, SLOPE = 2, 16, 8, 0.2
# The composed backward pass rounds y, dy and ds to float32 once each, where a float32 torch layer rounds everywhere: a gradient
# may differ from the float64 statement by four times what the float32 statement of the same layer (plain_grads in float32, on the
# CPU, the inputs of main) does: max |grad32 - grad64| / max |grad64| over the four gradients and both directions is 1.4e-6
# (xl.grad by row).
GRAD_TOL = 4 * 1.4e-6


def plain_grads(ops, G, rows, cols, by, dtype):
    """the gradients of the layer in plain torch, in `dtype`: gather, add, leaky_relu, (att * t).sum(-1), softmax per group, aggregate"""
    xl, xr, att, V = leaves = [x.detach().to(dtype).requires_grad_(True) for x in ops]
    grp, oth = (rows, cols) if by == "row" else (cols, rows)
    s = (att * torch.nn.functional.leaky_relu((xl[rows] + xr[cols]).view(-1, HEADS, D), SLOPE)).sum(-1)          # [edges, heads]
    m = torch.full((V.shape[0], HEADS), -torch.inf, dtype=dtype, device=s.device).scatter_reduce(0, grp[:, None].expand(-1, HEADS), s.detach(), "amax")
    p = torch.exp(s - m[grp])
    y = p / torch.zeros_like(m).index_add_(0, grp, p)[grp]
    out = torch.zeros((V.shape[0], HEADS, DV), dtype=dtype, device=s.device).index_add_(0, grp, y[:, :, None] * V[oth].view(-1, HEADS, DV))
    out.view(V.shape[0], HEADS * DV).backward(G.to(dtype))
    return [x.grad for x in leaves]


def main():
    import fora_amd
    from fora_amd import torch_ops
    dev, engine = torch.device("cuda", 0), fora_amd.Engine(0)
    row_ptr_g, col, U = sr.crafted_graph()
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(row_ptr_g, col, U)
    nc, rng = U.size, np.random.Generator(np.random.PCG64(10800))
    xl, xr, att, V, G = (rng.standard_normal(s).astype(np.float32) for s in ((nc, HEADS * D), (nc, HEADS * D), (HEADS, D), (nc, HEADS * DV), (nc, HEADS * DV)))
    engine.set_graph(sr.CRAFTED_N, int(row_ptr_g[-1]), row_ptr_g, col)
    engine.store_load(np.array([0, nc], dtype=np.int64), U, np.full(nc, 1 << 40, dtype=np.uint64))
    engine.set_option("attn_short", 64)                                         # both paths in every call
    engine.store_take_subgraph([0, 0])
    dn = lambda x: torch.from_numpy(x).to(dev)
    rows, cols = dn(np.repeat(np.arange(nc), np.diff(sub_ptr))), dn(np.asarray(sub_col, dtype=np.int64))
    for direction, by in (("out", "row"), ("in", "col")):
        wide = torch.zeros((nc, HEADS * (D + DV) + 5), device=dev)                  # column slices read in place, xl is xr, a pitched out64
        x_view, v_view = wide[:, 1:1 + HEADS * D], wide[:, 3 + HEADS * D:3 + HEADS * (D + DV)]
        x_view.copy_(dn(xl)), v_view.copy_(dn(V))
        buf = torch.full((nc, HEADS * DV + 3), 7.0, dtype=torch.float64, device=dev)
        _, _, y, _, st = engine.subgraph_gatv2(x_view, x_view, dn(att), v_view, heads=HEADS, by=by, want32=False, out64=buf[:, :HEADS * DV], want_y32=True)
        want = g2.forward(sub_ptr, sub_col, xl, xl, att, V, heads=HEADS, slope=SLOPE, by=by)
        assert y.is_cuda and st["long_groups"] == 6 and (buf[:, HEADS * DV:] == 7.0).all()
        same(buf[:, :HEADS * DV].contiguous(), want[0], f"a caller-made out64 {by}")
        same(y, want[3], f"y32 {by}")
        leaves = [dn(x).requires_grad_(True) for x in (xl, xr, att, V)]
        out = torch_ops.subgraph_gatv2(engine, *leaves, heads=HEADS, slope=SLOPE, direction=direction)
        same(out, g2.forward(sub_ptr, sub_col, xl, xr, att, V, heads=HEADS, slope=SLOPE, by=by)[1], f"forward {direction}")
        out.backward(dn(G))
        for leaf, w, name in zip(leaves, plain_grads(leaves, dn(G), rows, cols, by, torch.float64), ("xl", "xr", "att", "V")):
            err = float((leaf.grad.double() - w).abs().max() / w.abs().max())
            print(f"{name}.grad {direction}: {err:.3e} of the largest magnitude (allowed {GRAD_TOL:.1e})")
            assert leaf.grad.dtype == torch.float32 and err <= GRAD_TOL, (name, direction, err)
    engine.close()
    print("subgraph gatv2 device ok")


if __name__ == "__main__":
    main()
