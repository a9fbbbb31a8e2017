"""Child process of tests/test_subgraph_gatv2_bwd_gpu.py::test_device_tensors_and_autograd: torch_ops.subgraph_gatv2_trained on
device tensors against the twin, float64 autograd and itself.  torch is imported first: one HIP runtime in the process."""
import numpy as np
import torch

from subgraph_gatv2_device_child import DV, GRAD_TOL, HEADS, SLOPE, D, plain_grads  # (puts the repository and tests/ on sys.path)

import subgraph_gatv2_ref as g2  # noqa: E402
import subgraph_prop_ref as sr  # noqa: E402
import subgraph_ref  # noqa: E402
from subgraph_prop_device_child import same  # noqa: E402


def main():
    import fora_amd
    from fora_amd import torch_ops
    dev, engine = torch.device("cuda", 0), fora_amd.Engine(0)
    row_ptr_g, col, U = sr.crafted_graph()
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(row_ptr_g, col, U)
    nc, rng = U.size, np.random.Generator(np.random.PCG64(10950))
    xl, xr, att, V, G = (rng.standard_normal(s).astype(np.float32) for s in ((nc, HEADS * D), (nc, HEADS * D), (HEADS, D), (nc, HEADS * DV), (nc, HEADS * DV)))
    engine.set_graph(sr.CRAFTED_N, int(row_ptr_g[-1]), row_ptr_g, col)
    engine.store_load(np.array([0, nc], dtype=np.int64), U, np.full(nc, 1 << 40, dtype=np.uint64))
    engine.set_option("attn_short", 64)                                         # both paths on both sides in every call
    engine.store_take_subgraph([0, 0])
    dn = lambda x: torch.from_numpy(x).to(dev)
    rows, cols = dn(np.repeat(np.arange(nc), np.diff(sub_ptr))), dn(np.asarray(sub_col, dtype=np.int64))
    for direction, by in (("out", "row"), ("in", "col")):
        runs = []
        for _ in range(2):
            leaves = [dn(x).requires_grad_(True) for x in (xl, xr, att, V)]
            out = torch_ops.subgraph_gatv2_trained(engine, *leaves, heads=HEADS, slope=SLOPE, direction=direction)
            same(out, g2.forward(sub_ptr, sub_col, xl, xr, att, V, heads=HEADS, slope=SLOPE, by=by)[1], f"forward {direction}")
            out.backward(dn(G))
            runs.append([leaf.grad for leaf in leaves])
        assert engine.last_subgraph_gatv2_bwd["long_groups"] == 6 == engine.last_subgraph_gatv2_bwd["across_long"]
        for a, b, w, name in zip(*runs, plain_grads(leaves, dn(G), rows, cols, by, torch.float64), ("xl", "xr", "att", "V")):
            err = float((a.double() - w).abs().max() / w.abs().max())
            print(f"{name}.grad {direction}: {err:.3e} of the largest magnitude (allowed {GRAD_TOL:.1e})")
            assert a.dtype == torch.float32 and err <= GRAD_TOL, (name, direction, err)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}.grad {direction}: two runs differ"
    engine.close()
    print("subgraph gatv2_bwd device ok")


if __name__ == "__main__":
    main()
