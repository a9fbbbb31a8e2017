"""EDGE SOFTMAX (include/fora_hip_edge_softmax.h) checked on the CPU: the numpy twin (tests/subgraph_softmax_ref.py) by hand, and
the boundary -- the fifth header, the library, capi.ABI_EDGE_SOFTMAX, the Engine methods and the two torch functions."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import softmax_ref
import subgraph_ref
import subgraph_softmax_ref as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fora_hip_edge_softmax.h")
NAMES = ["fora_hip_subgraph_softmax", "fora_hip_subgraph_softmax_bwd"]
INF = np.inf


def test_twin_by_hand():
    # the four-node graph of test_subgraph_sddmm_cpu: the edges (0,1) (0,1) (0,0) (2,0) (2,2) -- rows {0,1,2} {} {3,4}, columns {2,3} {0,1} {4}
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(np.array([0, 3, 4, 4, 6]), np.array([1, 1, 0, 2, 0, 3]), [0, 1, 3])
    scores = np.array([[0, 0, -INF, 0, 0], [7, 7, 7, 1, np.nan]], dtype=np.float32)
    third, e3 = np.float64(1) / np.float64(3), softmax_ref.exp_def(np.float64(-3.0))[()]
    for by, want, nans in (("row", [[.5, .5, 0, .5, .5], [third, third, third, np.nan, np.nan]], 1),
                           ("col", [[.5, .5, 0, 1, 1], [.5, .5, 1 / (1 + e3), e3 / (1 + e3), np.nan]], 1)):
        out64, out32, nan_groups = sm.forward(sub_ptr, sub_col, scores, scale=0.5, by=by)
        assert np.array_equal(out64, np.array(want), equal_nan=True) and nan_groups == nans, by
        assert out64.dtype == np.float64 and out32.dtype == np.float32 and np.array_equal(out32, out64.astype(np.float32), equal_nan=True)
    y, g = np.array([[.5, .5, 0, .5, .5]]), np.array([[1, 3, 5, 2, 4]], dtype=np.float32)
    assert sm.backward(sub_ptr, sub_col, y, g, scale=2.0, by="row")[0].tolist() == [[-1, 1, 0, -1, 1]]      # D = 2 and 3
    assert sm.backward(sub_ptr, sub_col, y, g, scale=2.0, by="col")[0].tolist() == [[-1, 1, 0, 1, 2]]       # D = 1, 2 and 2


def test_header_library_and_binding_name_the_two_calls(tmp_path):
    import abi_header
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = abi_header.source(HEADER)
    assert "typedef" not in text and abi_header.structs(text) == {}
    declared = abi_header.prototypes(text, capi.STRUCTS)
    assert list(declared) == NAMES == capi.EDGE_SOFTMAX_SYMBOLS == list(capi.ABI_EDGE_SOFTMAX)
    raw = open(HEADER).read()
    assert '#include "fora_hip_edge.h"' in raw and "EDGE SOFTMAX" in raw and "#define FORA_SUB_BY_COL 2" in raw and capi.SUB_BY_COL == 2 != capi.SUB_MEAN
    lib = capi.load()
    for name in NAMES:
        test_only, restype, argtypes = capi.ABI_EDGE_SOFTMAX[name]
        assert not test_only and restype is declared[name][0] is ctypes.c_int and argtypes == declared[name][1]
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes == argtypes                # (load() bound the fifth table too)
    # the four older censuses are what they were
    assert (len(capi.ABI), len(capi.SYMBOLS), len(capi.ABI_EXT), len(capi.EXT_SYMBOLS), len(capi.ABI_GNN), len(capi.GNN_SYMBOLS)) == (68, 63, 2, 2, 3, 3)
    assert capi.EDGE_SYMBOLS == ["fora_hip_subgraph_sddmm"]
    assert not set(NAMES) & (set(capi.ABI) | set(capi.ABI_EXT) | set(capi.ABI_GNN) | set(capi.ABI_EDGE))
    x = (ctypes.c_float * 4)()
    assert lib.fora_hip_subgraph_softmax(None, x, 0, 1, 1.0, 0, x, None, 4, None, None) == -1          # a NULL ctx: answered without a GPU
    assert lib.fora_hip_subgraph_softmax_bwd(None, x, 0, x, 0, 1, 1.0, 0, x, None, 4, None, None) == -1
    assert list(inspect.signature(capi.Engine.subgraph_softmax).parameters) == ["self", "scores", "scale", "by", "want32", "want64", "out32", "out64"]
    assert list(inspect.signature(capi.Engine.subgraph_softmax_bwd).parameters) == ["self", "y", "g", "scale", "by", "want32", "want64", "out32", "out64"]
    src = tmp_path / "edge_softmax.c"                                                # the header is plain C99
    src.write_text('#include "fora_hip_edge_softmax.h"\nint main(void) { float x = 0; return fora_hip_subgraph_softmax(0, &x, FORA_PROP_F32, 1, 1.0, FORA_SUB_BY_COL, &x, 0, 1, 0, 0)'
                   ' + fora_hip_subgraph_softmax_bwd(0, &x, FORA_PROP_F32, &x, FORA_PROP_F64, 1, 1.0, 0, &x, 0, 1, 0, 0) + fora_hip_subgraph_sddmm(0, &x, 0, 1, &x, 0, 1, 1, 1, &x, 0, 1, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_torch_functions_are_there_with_their_refusals():
    import torch
    from fora_amd import torch_ops as t
    x, s = torch.zeros((2, 4)), torch.zeros((1, 3))
    assert list(inspect.signature(t.subgraph_edge_softmax).parameters) == ["engine", "scores", "scale", "by"]
    assert list(inspect.signature(t.subgraph_attention).parameters) == ["engine", "Q", "K", "V", "heads", "scale", "direction"]
    refused = [lambda: t.subgraph_edge_softmax(None, s, by="both"), lambda: t.subgraph_edge_softmax(None, s[0]),       # [heads, edges]
               lambda: t.subgraph_attention(None, x, x, x, heads=3), lambda: t.subgraph_attention(None, x, x, x, heads=0),
               lambda: t.subgraph_attention(None, x, x, x[:, :3], heads=2),                                            # heads divide V's columns too
               lambda: t.subgraph_attention(None, x, x, x, direction="both"),
               lambda: t.subgraph_attention(None, x, x.to(torch.float8_e5m2).requires_grad_(True), x)]                 # an FP8 leaf
    for call in refused:
        with pytest.raises(ValueError):
            call()
