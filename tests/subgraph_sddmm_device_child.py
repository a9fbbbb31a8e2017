"""Child process of tests/test_subgraph_sddmm_gpu.py::test_device_tensors_and_autograd: Engine.subgraph_sddmm over device tensors
read in place, torch_ops.subgraph_sddmm and torch_ops.subgraph_propagate_values with their backward passes.  torch is imported
first, so that the library binds to the HIP runtime torch brought along."""
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
import subgraph_sddmm_ref as ss  # noqa: E402
import fora_amd  # noqa: E402
from fora_amd import torch_ops  # noqa: E402
from subgraph_prop_device_child import same  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    engine = fora_amd.Engine(0)
    row_ptr_g, col, U = sr.crafted_graph()
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(row_ptr_g, col, U)
    nc, edges, d = U.size, sub_col.size, 8
    engine.set_graph(sr.CRAFTED_N, int(row_ptr_g[-1]), row_ptr_g, col)
    engine.store_load(np.array([0, nc], dtype=np.int64), U, np.full(nc, 1 << 40, dtype=np.uint64))
    engine.store_take_subgraph([0, 0])
    rng = np.random.Generator(np.random.PCG64(9970))
    dn = lambda x: torch.from_numpy(x).to(dev)
    mat = lambda w: pv.distinct_values(rng, nc * w, np.float32).reshape(nc, w)

    # ---- device tensors as column slices of wider tensors, one side on the host, a caller-made output
    for heads, dd in ((2, 8), (1, 33)):
        w = heads * dd
        A, B = mat(w), mat(w)
        w64, w32 = ss.scores(sub_ptr, sub_col, A, B, heads=heads)
        wa, wb = torch.zeros((nc, w + 5), device=dev), torch.zeros((nc, w + 3), device=dev)
        wa[:, 2:2 + w], wb[:, 3:3 + w] = dn(A), dn(B)
        o32, o64, st = engine.subgraph_sddmm(wa[:, 2:2 + w], wb[:, 3:3 + w], heads=heads, want64=True)
        assert o32.is_cuda and o64.is_cuda and st["a_on_device"] == st["b_on_device"] == 1
        same(o32, w32, "out32")
        same(o64, w64, "out64")
        o32, _, st = engine.subgraph_sddmm(A, wb[:, 3:3 + w], heads=heads)
        assert o32.is_cuda and (st["a_on_device"], st["b_on_device"]) == (0, 1)
        same(o32, w32, "a on the host")
        buf = torch.full((heads, edges), 7.0, dtype=torch.float64, device=dev)
        engine.subgraph_sddmm(wa[:, 2:2 + w], B, heads=heads, want32=False, out64=buf)
        same(buf, w64, "a caller-made out64")

    # ---- torch_ops.subgraph_sddmm: forward, and the gradients as the two products with values = g_h on the head's slice
    for heads in (1, 2):
        A, B = mat(heads * d), mat(heads * d)
        g = pv.distinct_values(rng, heads * edges, np.float32).reshape(heads, edges)
        Al, Bl = dn(A).requires_grad_(True), dn(B).requires_grad_(True)
        S = torch_ops.subgraph_sddmm(engine, Al, Bl, heads=heads)
        same(S, ss.scores(sub_ptr, sub_col, A, B, heads=heads)[1], f"forward, {heads} heads")
        S.backward(dn(g))
        for h in range(heads):
            cs = slice(h * d, (h + 1) * d)
            same(Al.grad[:, cs].contiguous(), sr.propagate(sub_ptr, sub_col, np.ascontiguousarray(B[:, cs]), values=g[h])[1], f"A.grad head {h}")
            same(Bl.grad[:, cs].contiguous(), sr.propagate_t(sub_ptr, sub_col, np.ascontiguousarray(A[:, cs]), values=g[h])[1], f"B.grad head {h}")

    # ---- torch_ops.subgraph_propagate_values: values.grad is the twin's scores of (G, X) or (X, G), X.grad the opposite product
    X, G, v = mat(d), mat(d), pv.distinct_values(rng, edges, np.float32)
    for direction, fwd, back, ab in (("out", sr.propagate, sr.propagate_t, (G, X)), ("in", sr.propagate_t, sr.propagate, (X, G))):
        Xl, vl = dn(X).requires_grad_(True), dn(v).requires_grad_(True)
        Y = torch_ops.subgraph_propagate_values(engine, Xl, vl, direction=direction)
        same(Y, fwd(sub_ptr, sub_col, X, values=v)[1], f"forward {direction}")
        Y.backward(dn(G))
        same(vl.grad, ss.scores(sub_ptr, sub_col, *ab)[1][0], f"values.grad {direction}")
        same(Xl.grad, back(sub_ptr, sub_col, G, values=v)[1], f"X.grad {direction}")

    # ---- float16 and bfloat16 leaves: read as they lie, the gradients come back in the leaf's dtype
    Xm, gm = rng.standard_normal((nc, d)).astype(np.float32), rng.standard_normal((1, edges)).astype(np.float32)   # (finite in float16)
    for dtype, kind in ((torch.float16, narrow_ref.F16), (torch.bfloat16, "bf16")):
        Al, Bl = dn(Xm).to(dtype).requires_grad_(True), dn(X).requires_grad_(True)
        codes = Al.detach().view(torch.int16).cpu().numpy().view(np.uint16)
        S = torch_ops.subgraph_sddmm(engine, Al, Bl)
        same(S, ss.scores(sub_ptr, sub_col, codes, X, a_kind=kind)[1], f"forward {dtype}")
        S.backward(dn(gm))
        want = torch.from_numpy(sr.propagate(sub_ptr, sub_col, X, values=gm[0])[1]).to(dtype)
        assert Al.grad.dtype == dtype and torch.equal(Al.grad.cpu().view(torch.int16), want.view(torch.int16))
        same(Bl.grad, sr.propagate_t(sub_ptr, sub_col, codes, values=gm[0], kind=kind)[1], f"B.grad beside a {dtype} leaf")

    # ---- the generation guard, for both functions
    for make in (lambda: torch_ops.subgraph_sddmm(engine, dn(X).requires_grad_(True), dn(G)).sum(),
                 lambda: torch_ops.subgraph_propagate_values(engine, dn(X), dn(v).requires_grad_(True)).sum()):
        loss = make()
        engine.store_take_subgraph([0, 0])                                      # the held result was replaced (by an equal one)
        try:
            loss.backward()
            raise AssertionError("a backward pass after the held result was replaced went through")
        except RuntimeError as e:
            assert "replaced or cleared" in str(e)
    engine.close()
    print("subgraph sddmm device ok")


if __name__ == "__main__":
    main()
