"""Child process of tests/test_subgraph_pool_gpu.py::test_device_tensors_and_autograd: Engine.subgraph_pool and subgraph_pool_bwd over
device tensors in place, and torch_ops.subgraph_pool with its backward pass.  torch is imported first (one HIP runtime)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import propagate_values_ref as pv  # noqa: E402
import subgraph_pool_ref as pool  # noqa: E402
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
    nc, d = U.size, 8
    engine.set_graph(sr.CRAFTED_N, int(row_ptr_g[-1]), row_ptr_g, col)
    engine.store_load(np.array([0, nc], dtype=np.int64), U, np.full(nc, 1 << 40, dtype=np.uint64))
    engine.set_option("sub_short", 64)                                         # both paths in every call
    engine.set_option("prop_segs", 2)
    engine.store_take_subgraph([0, 0])
    rng = np.random.Generator(np.random.PCG64(11350))
    X = rng.choice(np.array([-2, -1, -0.0, 0.0, 1, 2], dtype=np.float32), size=(nc, d))
    G = pv.distinct_values(rng, nc * d, np.float32).reshape(nc, d)
    Gt = torch.from_numpy(G).to(dev)

    # ---- column slices read in place at an odd and an even pitch, the outputs and arg written into slices
    for width, at in ((11, 1), (16, 4)):
        wide = torch.zeros((nc, width), dtype=torch.float32, device=dev)
        wide[:, at:at + d] = torch.from_numpy(X).to(dev)
        Xs = wide[:, at:at + d]
        for by in ("row", "col"):
            w64, w32, warg = pool.forward(sub_ptr, sub_col, X, op="min", by=by)
            buf, abuf = torch.full((nc, width), 7.0, dtype=torch.float32, device=dev), torch.full((nc, width), 7, dtype=torch.int32, device=dev)
            o64 = engine.subgraph_pool(Xs, op="min", by=by, want32=False, want64=True, want_arg=False)[1]
            o32, _, arg, st = engine.subgraph_pool(Xs, op="min", by=by, out32=buf[:, at:at + d], arg=abuf[:, at:at + d])
            assert o64.is_cuda and arg.is_cuda and st["x_on_device"] == 1 and st["long_rows"] == 6
            same(o64, w64, "out64 alone")
            same(buf[:, at:at + d].contiguous(), w32, "out32 in a slice")
            same(abuf[:, at:at + d].contiguous(), warg, "arg in a slice")
            assert (buf[:, :at] == 7.0).all() and (buf[:, at + d:] == 7.0).all() and (abuf[:, :at] == 7).all() and (abuf[:, at + d:] == 7).all()
            gw = torch.zeros((nc, width), dtype=torch.float32, device=dev)
            gw[:, at:at + d] = Gt
            b32, b64, _ = engine.subgraph_pool_bwd(gw[:, at:at + d], abuf[:, at:at + d], by=by, want64=True)   # (arg at a pitch: one word a load or four)
            d64, d32 = pool.backward(sub_ptr, sub_col, G, warg, by=by)
            same(b64, d64, "backward out64")
            same(b32, d32, "backward out32")

    # ---- autograd: both directions and both ops, the backward pass is the twin's over the twin's arg
    for direction, by in (("out", "row"), ("in", "col")):
        for op in ("max", "min"):
            w64, w32, warg = pool.forward(sub_ptr, sub_col, X, op=op, by=by)
            Xl = torch.from_numpy(X).to(dev).requires_grad_(True)
            Y = torch_ops.subgraph_pool(engine, Xl, op=op, direction=direction)
            same(Y, w32, f"forward {direction} {op}")
            Y.backward(Gt)
            same(Xl.grad, pool.backward(sub_ptr, sub_col, G, warg, by=by)[1], f"backward {direction} {op}")

    # ---- a bfloat16 leaf: read as it lies, the gradient comes back in the leaf's dtype
    Xn = torch.from_numpy(rng.standard_normal((nc, d)).astype(np.float32)).to(dev).to(torch.bfloat16)
    codes = Xn.view(torch.int16).cpu().numpy().view(np.uint16)
    Xl = Xn.clone().requires_grad_(True)
    Y = torch_ops.subgraph_pool(engine, Xl)
    w64, w32, warg = pool.forward(sub_ptr, sub_col, codes, kind="bf16")
    same(Y, w32, "forward bfloat16")
    Y.backward(Gt)
    want = torch.from_numpy(pool.backward(sub_ptr, sub_col, G, warg)[1]).to(torch.bfloat16)
    assert Xl.grad.dtype == torch.bfloat16 and torch.equal(Xl.grad.cpu().view(torch.int16), want.view(torch.int16))

    # ---- the refusal after the held rows were replaced
    Xl = torch.from_numpy(X).to(dev).requires_grad_(True)
    Y = torch_ops.subgraph_pool(engine, Xl)
    engine.store_take_subgraph([0, 0])                                          # (by an equal result)
    try:
        Y.backward(Gt)
        raise AssertionError("a backward pass after the held result was replaced went through")
    except RuntimeError as e:
        assert "replaced or cleared" in str(e)
    engine.close()
    print("subgraph pool device ok")


if __name__ == "__main__":
    main()
