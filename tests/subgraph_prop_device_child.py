"""Child process of tests/test_subgraph_prop_gpu.py::test_device_tensors_and_autograd: Engine.subgraph_propagate and
subgraph_propagate_t over device tensors read and written in place, and torch_ops.subgraph_propagate with its backward pass.
torch is imported first, so that the library binds to the HIP runtime torch brought along and a tensor's data_ptr() is device
memory the library knows."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import narrow_ref  # noqa: E402
import propagate_values_ref as pv  # noqa: E402
import subgraph_prop_ref as sr  # noqa: E402
import subgraph_ref  # noqa: E402
import fora_amd  # noqa: E402
from fora_amd import torch_ops  # noqa: E402


def same(t, want, name):
    got = t.detach().cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    assert (got.view(np.uint8) == want.view(np.uint8)).all(), name


def main():
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    engine = fora_amd.Engine(0)
    row_ptr_g, col, U = sr.crafted_graph()
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(row_ptr_g, col, U)
    nc, edges, d = U.size, sub_col.size, 8
    engine.set_graph(sr.CRAFTED_N, int(row_ptr_g[-1]), row_ptr_g, col)
    engine.store_load(np.array([0, nc], dtype=np.int64), U, np.full(nc, 1 << 40, dtype=np.uint64))
    engine.set_option("sub_short", 64)                                         # both paths in every call
    engine.set_option("prop_segs", 2)
    engine.store_take_subgraph([0, 0])
    rng = np.random.Generator(np.random.PCG64(9950))
    X = pv.distinct_values(rng, nc * d, np.float32).reshape(nc, d)
    G = pv.distinct_values(rng, nc * d, np.float32).reshape(nc, d)
    v32 = pv.distinct_values(rng, edges, np.float32)
    fwd, tr = sr.propagate(sub_ptr, sub_col, X), sr.propagate_t(sub_ptr, sub_col, X)
    counts = {"out": np.diff(sub_ptr), "in": np.bincount(sub_col, minlength=nc)}

    # ---- column slices read in place at an odd and an even pitch (one lane a column; four columns a lane), outputs at a pitch
    for width, at in ((11, 1), (16, 4)):
        wide = torch.zeros((nc, width), dtype=torch.float32, device=dev)
        wide[:, at:at + d] = torch.from_numpy(X).to(dev)
        Xs = wide[:, at:at + d]
        for fn, (w64, w32) in ((engine.subgraph_propagate, fwd), (engine.subgraph_propagate_t, tr)):
            o32, o64, st = fn(Xs, want32=True, want64=True)
            assert o32.is_cuda and o64.is_cuda and st["x_on_device"] == 1 and st["long_rows"] == 6
            same(o32, w32, "out32")
            same(o64, w64, "out64")
            buf = torch.full((nc, width), 7.0, dtype=torch.float32, device=dev)
            fn(Xs, want64=False, out32=buf[:, at:at + d])
            same(buf[:, at:at + d].contiguous(), w32, "out32 in a slice")
            assert (buf[:, :at] == 7.0).all() and (buf[:, at + d:] == 7.0).all()
        vt = torch.from_numpy(v32).to(dev)
        same(engine.subgraph_propagate(Xs, values=vt)[0], sr.propagate(sub_ptr, sub_col, X, values=v32)[1], "values on the device")
        same(engine.subgraph_propagate_t(Xs, values=vt)[0], sr.propagate_t(sub_ptr, sub_col, X, values=v32)[1], "values on the device, transposed")
    for a, b in zip(engine.subgraph_transpose_fetch(device=True), sr.transpose(sub_ptr, sub_col)):
        assert a.is_cuda
        same(a, b, "the transposition on the device")

    # ---- autograd: both directions, the backward pass is the twin's opposite product of G
    Gt = torch.from_numpy(G).to(dev)
    for direction, (w64, w32), back in (("out", fwd, sr.propagate_t), ("in", tr, sr.propagate)):
        Xl = torch.from_numpy(X).to(dev).requires_grad_(True)
        Y = torch_ops.subgraph_propagate(engine, Xl, direction=direction)
        same(Y, w32, f"forward {direction}")
        Y.backward(Gt)
        same(Xl.grad, back(sub_ptr, sub_col, G)[1], f"backward {direction}")
        # with values: a constant, used in both passes
        Xl = torch.from_numpy(X).to(dev).requires_grad_(True)
        Y = torch_ops.subgraph_propagate(engine, Xl, values=torch.from_numpy(v32).to(dev), direction=direction)
        same(Y, (sr.propagate if direction == "out" else sr.propagate_t)(sub_ptr, sub_col, X, values=v32)[1], f"forward {direction} with values")
        Y.backward(Gt)
        same(Xl.grad, back(sub_ptr, sub_col, G, values=v32)[1], f"backward {direction} with values")
        # norm="mean": the stated composition -- G's rows divided by the forward counts in torch, then the plain opposite call
        Xl = torch.from_numpy(X).to(dev).requires_grad_(True)
        Y = torch_ops.subgraph_propagate(engine, Xl, norm="mean", direction=direction)
        same(Y, (sr.propagate if direction == "out" else sr.propagate_t)(sub_ptr, sub_col, X, mean=True)[1], f"forward {direction} mean")
        Y.backward(Gt)
        same(Xl.grad, back(sub_ptr, sub_col, sr.mean_backward_operand(G, counts[direction]))[1], f"backward {direction} mean")

    # ---- float16 and bfloat16 leaves: read as they lie, the gradient comes back in the leaf's dtype
    Xm = rng.standard_normal((nc, d)).astype(np.float32)                        # (finite in float16)
    for dtype, kind in ((torch.float16, narrow_ref.F16), (torch.bfloat16, "bf16")):
        Xn = torch.from_numpy(Xm).to(dev).to(dtype)
        codes = Xn.view(torch.int16).cpu().numpy().view(np.uint16)
        Xl = Xn.clone().requires_grad_(True)
        Y = torch_ops.subgraph_propagate(engine, Xl)
        same(Y, sr.propagate(sub_ptr, sub_col, codes, kind=kind)[1], f"forward {dtype}")
        Y.backward(torch.from_numpy(Xm).to(dev))
        want = torch.from_numpy(sr.propagate_t(sub_ptr, sub_col, Xm)[1]).to(dtype)
        assert Xl.grad.dtype == dtype and torch.equal(Xl.grad.cpu().view(torch.int16), want.view(torch.int16))

    # ---- the three refusals
    x8 = torch.from_numpy(X).to(dev).clamp(-100, 100).to(torch.float8_e4m3fn)
    same(torch_ops.subgraph_propagate(engine, x8), sr.propagate(sub_ptr, sub_col, x8.view(torch.uint8).cpu().numpy(), kind=narrow_ref.E4M3)[1], "FP8 constant")
    try:
        torch_ops.subgraph_propagate(engine, x8.requires_grad_(True))
        raise AssertionError("an FP8 tensor that requires grad was accepted")
    except ValueError:
        pass
    try:
        torch_ops.subgraph_propagate(engine, torch.from_numpy(X).to(dev), values=torch.from_numpy(v32).to(dev).requires_grad_(True))
        raise AssertionError("values that require grad were accepted")
    except ValueError:
        pass
    Xl = torch.from_numpy(X).to(dev).requires_grad_(True)
    Y = torch_ops.subgraph_propagate(engine, Xl)
    engine.store_take_subgraph([0, 0])                                          # the held result was replaced (by an equal one)
    try:
        Y.backward(Gt)
        raise AssertionError("a backward pass after the held result was replaced went through")
    except RuntimeError as e:
        assert "replaced or cleared" in str(e)
    engine.sparse_clear()
    try:
        engine.subgraph_propagate(torch.from_numpy(X).to(dev))
        raise AssertionError("a call without a held subgraph went through")
    except fora_amd.capi.ForaError:
        pass
    engine.close()
    print("subgraph products device ok")


if __name__ == "__main__":
    main()
