"""EDGE GATV2 (include/fora_hip_edge_gatv2.h) checked on the CPU: the numpy twin (tests/subgraph_gatv2_ref.py) by hand, and the
boundary -- the tenth header, the library, capi.ABI_EDGE_GATV2, the Engine method and the torch function."""
import ctypes
import os

import numpy as np
import pytest

import subgraph_gatv2_ref as g2
import subgraph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fora_hip_edge_gatv2.h")
NAME = "fora_hip_subgraph_gatv2"


def test_twin_by_hand():
    # the four-node graph of test_subgraph_gat_cpu: the edges (0,1) (0,1) (0,0) (2,0) (2,2) -- rows {0,1,2} {} {3,4}, columns {2,3} {0,1} {4}
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(np.array([0, 3, 4, 4, 6]), np.array([1, 1, 0, 2, 0, 3]), [0, 1, 3])
    f = lambda *rows: np.array(rows, dtype=np.float32)
    xl, xr, att, V = f([1, -0.0], [7, 7], [-3, 1]), f([1, -0.0], [2, 3], [-1, np.nan]), f([2, .5]), f([1], [2], [4])
    # u = xl[row] + xr[col]: (3 3) (3 3) (2 -0.0) (-2 1) (-4 NaN); slope .5: t = (3 3) (3 3) (2 -0.0) (-1 1) (-2 NaN);
    # att * t = (6 1.5) (6 1.5) (4 -0.0) (-2 .5) (-4 NaN); q_0 + q_1, each from +0.0: 7.5 7.5 4 -1.5 NaN -- whichever the grouping
    s = g2.scores(sub_ptr, sub_col, xl, xr, att, slope=0.5)
    assert s[0, :4].tolist() == [7.5, 7.5, 4, -1.5] and np.isnan(s[0, 4]) and not np.signbit(s[0, 2])
    out, out32, y, _, nan = g2.forward(sub_ptr, sub_col, xl, xr, att, V, slope=0.5, by="row")    # row 2 holds the NaN: written, counted
    assert nan == 1 and np.isnan(y[0, 3:]).all() and np.isnan(out[2, 0]) and out[1, 0] == 0 and np.array_equal(out32, out.astype(np.float32), equal_nan=True)
    out, _, y, _, nan = g2.forward(sub_ptr, sub_col, xl, xr, att, V, slope=0.5, by="col")        # columns {2,3} {0,1} {4}; v at the rows
    assert nan == 1 and y[0, :2].tolist() == [.5, .5] and out[1, 0] == .5 * 1 + .5 * 1 and np.isnan(out[2, 0]) and 0 < y[0, 3] < y[0, 2] < 1


def test_header_library_binding_and_torch_refusals():
    import abi_header
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = abi_header.source(HEADER)
    assert "typedef" not in text and abi_header.structs(text) == {}
    declared = abi_header.prototypes(text, capi.STRUCTS)
    assert list(declared) == [NAME] == capi.EDGE_GATV2_SYMBOLS == list(capi.ABI_EDGE_GATV2)
    lib = capi.load()
    test_only, restype, argtypes = capi.ABI_EDGE_GATV2[NAME]
    assert not test_only and restype is declared[NAME][0] is ctypes.c_int and argtypes == declared[NAME][1] and len(argtypes) == 26
    fn = getattr(lib, NAME)
    assert fn.restype is ctypes.c_int and fn.argtypes == argtypes                    # (load() bound the tenth table too)
    x = (ctypes.c_float * 4)()
    assert fn(None, x, 0, 1, x, 0, 1, x, 0, 1, x, 0, 1, 1, 1, 1, 0.2, 0, x, None, 1, None, None, 0, None, None) == -1   # a NULL ctx: answered without a GPU
    # ---- the torch function and its refusals
    import torch
    from fora_amd import torch_ops as t
    x, a = torch.zeros((2, 4)), torch.zeros((2, 2))
    refused = [lambda: t.subgraph_gatv2(None, x, x, a, x, heads=2, direction="both"), lambda: t.subgraph_gatv2(None, x, x, a, x, heads=3),   # 3 does not divide 4
               lambda: t.subgraph_gatv2(None, x, x, a, x[:, :3], heads=2), lambda: t.subgraph_gatv2(None, x, x[:, :2], a, x, heads=2),
               lambda: t.subgraph_gatv2(None, x, x, a.T[:1], x, heads=2), lambda: t.subgraph_gatv2(None, x, x, a[0], x, heads=2),              # att is [heads, d]
               lambda: t.subgraph_gatv2(None, x, x, a.to(torch.float8_e5m2).requires_grad_(True), x, heads=2)]                                 # an FP8 leaf
    for call in refused:
        with pytest.raises(ValueError):
            call()
