"""EDGE ATTENTION (include/fora_hip_edge_attention.h) checked on the CPU: the numpy twin (tests/subgraph_attention_ref.py) by hand,
and the boundary -- the sixth header, the library, capi.ABI_EDGE_ATTENTION, the Engine method and the torch function."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import subgraph_attention_ref as at
import subgraph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fora_hip_edge_attention.h")
NAME = "fora_hip_subgraph_attention"


def test_twin_by_hand():
    # the four-node graph of test_subgraph_sddmm_cpu: the edges (0,1) (0,1) (0,0) (2,0) (2,2) -- rows {0,1,2} {} {3,4}, columns {2,3} {0,1} {4}
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(np.array([0, 3, 4, 4, 6]), np.array([1, 1, 0, 2, 0, 3]), [0, 1, 3])
    Q, K, V = np.zeros((3, 2), np.float32), np.ones((3, 2), np.float32), np.array([[3, 1], [6, 1], [12, 1]], dtype=np.float32)
    t = np.float64(1) / np.float64(3)
    for by, y, out in (("row", [t, t, t, .5, .5], [(t * 6 + t * 6) + t * 3, 0, .5 * 3 + .5 * 12]), ("col", [.5, .5, .5, .5, 1], [7.5, 3, 12])):
        out64, out32, y64, y32, nan_pairs = at.attention(sub_ptr, sub_col, Q, K, V, heads=2, scale=0.5, by=by)   # every score 0: uniform groups
        assert y64.tolist() == [y, y] and out64[:, 0].tolist() == out and nan_pairs == 0, by
        assert out64[:, 1].tolist() == [1 if by == "col" else (t + t) + t, 0 if by == "row" else 1, 1] and not np.signbit(out64[1]).any()
        assert out32.dtype == y32.dtype == np.float32 and np.array_equal(out32, out64.astype(np.float32)) and np.array_equal(y32, y64.astype(np.float32))
    K[1, 1] = np.nan                                               # head 1 of node 1's key: the row group of node 0 reads it, no column group does
    out64, _, y64, _, nan_pairs = at.attention(sub_ptr, sub_col, Q, K, V, heads=2, by="row")
    assert nan_pairs == 1 and np.isnan(y64[1, :3]).all() and np.isnan(out64[0, 1]) and not np.isnan(out64[:, 0]).any() and out64[2, 1] == 1
    assert out64.view(np.uint64)[0, 1] == 0x7FF8000000000000 and at.attention(sub_ptr, sub_col, Q, K, V, heads=2, by="col")[4] == 0


def test_header_library_and_binding_name_the_call(tmp_path):
    import abi_header
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = abi_header.source(HEADER)
    assert "typedef" not in text and abi_header.structs(text) == {}
    declared = abi_header.prototypes(text, capi.STRUCTS)
    assert list(declared) == [NAME] == capi.EDGE_ATTENTION_SYMBOLS == list(capi.ABI_EDGE_ATTENTION)
    raw = open(HEADER).read()
    assert '#include "fora_hip_edge_softmax.h"' in raw and "EDGE ATTENTION" in raw
    lib = capi.load()
    test_only, restype, argtypes = capi.ABI_EDGE_ATTENTION[NAME]
    assert not test_only and restype is declared[NAME][0] is ctypes.c_int and argtypes == declared[NAME][1] and len(argtypes) == 23
    fn = getattr(lib, NAME)
    assert fn.restype is ctypes.c_int and fn.argtypes == argtypes                    # (load() bound the sixth table too)
    assert len(capi.ABI_EDGE_SOFTMAX) == 2 and NAME not in set(capi.ABI) | set(capi.ABI_EXT) | set(capi.ABI_GNN) | set(capi.ABI_EDGE) | set(capi.ABI_EDGE_SOFTMAX)
    x = (ctypes.c_float * 4)()
    assert fn(None, x, 0, 1, x, 0, 1, x, 0, 1, 1, 1, 1, 1.0, 0, x, None, 1, None, None, 0, None, None) == -1   # a NULL ctx: answered without a GPU
    assert list(inspect.signature(capi.Engine.subgraph_attention).parameters)[:11] == ["self", "Q", "K", "V", "heads", "scale", "by", "want32", "want64", "want_y32", "want_y64"]
    src = tmp_path / "edge_attention.c"                                              # the header is plain C99
    src.write_text('#include "fora_hip_edge_attention.h"\nint main(void) { float x = 0; return fora_hip_subgraph_attention(0, &x, FORA_PROP_F32, 1, &x, FORA_PROP_BF16, 1, &x, '
                   'FORA_PROP_E4M3, 1, 1, 1, 1, 1.0, FORA_SUB_BY_COL, &x, 0, 1, 0, 0, 0, 0, 0) + fora_hip_subgraph_softmax(0, &x, FORA_PROP_F32, 1, 1.0, 0, &x, 0, 1, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_torch_function_is_there_with_its_refusals():
    import torch
    from fora_amd import torch_ops as t
    x = torch.zeros((2, 4))
    assert list(inspect.signature(t.subgraph_attention_fused).parameters) == ["engine", "Q", "K", "V", "heads", "scale", "direction"]
    refused = [lambda: t.subgraph_attention_fused(None, x, x, x, heads=3), lambda: t.subgraph_attention_fused(None, x, x, x, heads=0),
               lambda: t.subgraph_attention_fused(None, x, x, x[:, :3], heads=2),                                      # heads divide V's columns too
               lambda: t.subgraph_attention_fused(None, x, x[:, :2], x), lambda: t.subgraph_attention_fused(None, x, x, x, direction="both"),
               lambda: t.subgraph_attention_fused(None, x, x.to(torch.float8_e5m2).requires_grad_(True), x)]           # an FP8 leaf
    for call in refused:
        with pytest.raises(ValueError):
            call()
