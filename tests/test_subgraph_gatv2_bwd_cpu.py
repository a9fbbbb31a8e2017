"""EDGE GATV2, BACKWARD (include/fora_hip_edge_gatv2_bwd.h) checked on the CPU: the numpy twin (tests/subgraph_gatv2_bwd_ref.py)
against float64 autograd, and the boundary -- the eleventh header, the library, capi.ABI_EDGE_GATV2_BWD, the Engine method and the
torch function."""
import ctypes
import os

import numpy as np
import pytest

import subgraph_gatv2_bwd_ref as g2b
import subgraph_gatv2_ref as g2
import subgraph_prop_ref as sr
import subgraph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fora_hip_edge_gatv2_bwd.h")
NAME = "fora_hip_subgraph_gatv2_bwd"


@pytest.mark.parametrize("by", ["row", "col"])
def test_twin_against_float64_autograd(by):
    import __graft_entry__
    __graft_entry__.build()                      # (the child module imports the package)
    import torch
    import subgraph_gatv2_device_child as child
    row_ptr_g, col, U = sr.crafted_graph()
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(row_ptr_g, col, U)
    nc, rng, (H, D, DV) = U.size, np.random.Generator(np.random.PCG64(10900)), (child.HEADS, child.D, child.DV)
    xl, xr, att, V, G = ops = [rng.standard_normal(s).astype(np.float32) for s in ((nc, H * D), (nc, H * D), (H, D), (nc, H * DV), (nc, H * DV))]
    y64 = g2.forward(sub_ptr, sub_col, xl, xr, att, V, heads=H, slope=child.SLOPE, by=by)[2]
    got = g2b.backward(sub_ptr, sub_col, xl, xr, att, V, G, y64, heads=H, slope=child.SLOPE, by=by)[::2]
    rows, cols = torch.from_numpy(np.repeat(np.arange(nc), np.diff(sub_ptr))), torch.from_numpy(np.asarray(sub_col, dtype=np.int64))
    want = child.plain_grads([torch.from_numpy(x) for x in ops[:4]], torch.from_numpy(G), rows, cols, by, torch.float64)
    # The two sides differ only by the order of float64 additions (and the last bits of exp).  The longest chain is d att's: one
    # term per edge, each behind a softmax sum over its group -- n additions, each off by at most 2^-53 of the running magnitude.
    n = len(sub_col) + max(sr.LENS)
    for g, w, name in zip(got, want, ("xl", "xr", "att", "V")):
        err = float(np.abs(g - w.numpy()).max() / np.abs(w.numpy()).max())
        print(f"{name}.grad {by}: {err:.3e} of the largest magnitude (allowed {n * 2.0 ** -53:.1e})")
        assert err <= n * 2.0 ** -53, (name, by, err)


def test_header_library_binding_and_torch_function():
    import abi_header
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = abi_header.source(HEADER)
    assert "typedef" not in text and abi_header.structs(text) == {}
    declared = abi_header.prototypes(text, capi.STRUCTS)
    assert list(declared) == [NAME] == capi.EDGE_GATV2_BWD_SYMBOLS == list(capi.ABI_EDGE_GATV2_BWD)
    lib = capi.load()
    test_only, restype, argtypes = capi.ABI_EDGE_GATV2_BWD[NAME]
    assert not test_only and restype is declared[NAME][0] is ctypes.c_int and argtypes == declared[NAME][1] and len(argtypes) == 30
    fn = getattr(lib, NAME)
    assert fn.restype is ctypes.c_int and fn.argtypes == argtypes                    # (load() bound the eleventh table too)
    x = (ctypes.c_float * 4)()
    assert fn(None, *(x, 0, 1) * 5, x, 0, 4, 1, 1, 1, 0.2, 0, None, x, None, 1, None, None) == -1   # a NULL ctx: answered without a GPU
    import torch
    from fora_amd import torch_ops as t
    assert callable(capi.Engine.subgraph_gatv2_bwd) and issubclass(t._SubgraphGatv2Trained, t._SubgraphGatv2)
    x, a = torch.zeros((2, 4)), torch.zeros((2, 2))
    for call in (lambda: t.subgraph_gatv2_trained(None, x, x, a, x, heads=2, direction="both"), lambda: t.subgraph_gatv2_trained(None, x, x, a[0], x, heads=2)):
        with pytest.raises(ValueError):
            call()
