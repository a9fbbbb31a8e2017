"""EDGE SCORES (include/fora_hip_edge.h) checked on the CPU: the numpy twin (tests/subgraph_sddmm_ref.py) by hand, and the
boundary -- the fourth header, the library, capi.ABI_EDGE, the Engine method and the two torch functions."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import subgraph_ref
import subgraph_sddmm_ref as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_HEADER = os.path.join(ROOT, "include", "fora_hip_edge.h")
NAME = "fora_hip_subgraph_sddmm"


def test_twin_by_hand():
    # the four-node graph of test_subgraph_cpu.test_twin_rules: 0 -> 1, 1, 0; 1 -> 2; 2 -> nothing; 3 -> 0, 3; U = {0, 1, 3}
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(np.array([0, 3, 4, 4, 6]), np.array([1, 1, 0, 2, 0, 3]), [0, 1, 3])
    assert sub_ptr.tolist() == [0, 3, 3, 5] and sub_col.tolist() == [1, 1, 0, 0, 2]
    A = np.array([[1, 2, 3, 4], [np.nan] * 4, [5, 6, 7, 8]], dtype=np.float32)      # local row 1 has no edge: never read
    B = np.array([[1, 10, 100, 1000], [2, 20, 200, 2000], [3, 30, 300, 3000]], dtype=np.float32)
    out64, out32 = ss.scores(sub_ptr, sub_col, A, B, heads=2)
    # head 0 is columns 0, 1 and head 1 columns 2, 3; the edges are (0,1) (0,1) (0,0) (2,0) (2,2): a read at the ROW, b at the target
    assert out64.tolist() == [[42.0, 42.0, 21.0, 65.0, 195.0], [8600.0, 8600.0, 4300.0, 8700.0, 26100.0]]
    assert out64.dtype == np.float64 and out32.dtype == np.float32 and (out32 == out64.astype(np.float32)).all()
    assert ss.scores(sub_ptr, sub_col, A, B, heads=1)[0].tolist() == [(out64[0] + out64[1]).tolist()]


def test_edge_header_library_and_binding_name_the_one_call(tmp_path):
    import abi_header
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = abi_header.source(EDGE_HEADER)
    assert "typedef" not in text and abi_header.structs(text) == {}
    declared = abi_header.prototypes(text, capi.STRUCTS)
    assert list(declared) == [NAME] == capi.EDGE_SYMBOLS == list(capi.ABI_EDGE)
    test_only, restype, argtypes = capi.ABI_EDGE[NAME]
    assert not test_only and restype is declared[NAME][0] is ctypes.c_int and argtypes == declared[NAME][1]
    assert '#include "fora_hip_gnn.h"' in open(EDGE_HEADER).read() and "EDGE SCORES" in open(EDGE_HEADER).read()
    # the three older censuses are what they were
    assert (len(capi.ABI), len(capi.SYMBOLS), len(capi.ABI_EXT), len(capi.EXT_SYMBOLS), len(capi.ABI_GNN), len(capi.GNN_SYMBOLS)) == (68, 63, 2, 2, 3, 3)
    assert NAME not in set(capi.ABI) | set(capi.ABI_EXT) | set(capi.ABI_GNN)
    assert not any(NAME in abi_header.source(os.path.join(ROOT, "include", h)) for h in ("fora_hip.h", "fora_hip_ext.h", "fora_hip_gnn.h"))
    fn = getattr(capi.load(), NAME)
    assert fn.restype is ctypes.c_int and fn.argtypes == argtypes                    # (load() bound the fourth table too)
    x = (ctypes.c_float * 4)()
    assert fn(None, x, 0, 1, x, 0, 1, 1, 1, x, None, 4, None, None) == -1            # a NULL ctx: answered without a GPU
    assert list(inspect.signature(capi.Engine.subgraph_sddmm).parameters) == ["self", "a", "b", "heads", "want32", "want64", "out32", "out64", "a_bf16", "b_bf16"]
    src = tmp_path / "edge.c"                                                        # the header is plain C99
    src.write_text('#include "fora_hip_edge.h"\nint main(void) { float x = 0; return fora_hip_subgraph_sddmm(0, &x, FORA_PROP_F32, 1, &x, FORA_PROP_BF16, 1, 1, 1, &x, 0, 1, 0, 0)'
                   ' + fora_hip_subgraph_transpose_fetch(0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_torch_functions_are_there_with_their_refusals():
    import torch
    from fora_amd import torch_ops as t
    x, v = torch.zeros((2, 4)), torch.zeros(3)
    assert list(inspect.signature(t.subgraph_sddmm).parameters) == ["engine", "A", "B", "heads"]
    assert list(inspect.signature(t.subgraph_propagate_values).parameters) == ["engine", "X", "values", "direction"]
    refused = [lambda: t.subgraph_sddmm(None, x, x, heads=3), lambda: t.subgraph_sddmm(None, x, x, heads=0),             # heads divide the columns
               lambda: t.subgraph_sddmm(None, x, x.to(torch.float8_e5m2).requires_grad_(True)),                          # an FP8 leaf
               lambda: t.subgraph_propagate_values(None, x.to(torch.float8_e4m3fn).requires_grad_(True), v),
               lambda: t.subgraph_propagate_values(None, x, v, direction="both"),
               lambda: t.subgraph_propagate_values(None, x, v.double())]                                                  # values are float32
    for call in refused:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="subgraph_propagate_values"):               # the older function keeps its refusal and names the new one
        t.subgraph_propagate(None, x, values=v.clone().requires_grad_(True))
    assert "subgraph_propagate_values" in t.subgraph_propagate.__doc__
