"""EDGE ATTENTION, BACKWARD (include/fora_hip_edge_attention_bwd.h) checked on the CPU: the numpy twin
(tests/subgraph_attention_bwd_ref.py) by hand, and the boundary -- the seventh header, the library, capi.ABI_EDGE_ATTENTION_BWD, the
Engine method and the torch function."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import subgraph_attention_bwd_ref as bw
import subgraph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fora_hip_edge_attention_bwd.h")
NAME = "fora_hip_subgraph_attention_bwd"


def test_twin_by_hand():
    # the four-node graph of test_subgraph_attention_cpu: the edges (0,1) (0,1) (0,0) (2,0) (2,2) -- rows {0,1,2} {} {3,4}, columns {2,3} {0,1} {4}
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(np.array([0, 3, 4, 4, 6]), np.array([1, 1, 0, 2, 0, 3]), [0, 1, 3])
    Q, K = np.array([[1], [2], [4]], dtype=np.float32), np.array([[8], [16], [32]], dtype=np.float32)
    V, G = np.array([[1], [2], [3]], dtype=np.float32), np.array([[1], [0], [2]], dtype=np.float32)
    y = np.full((1, 5), 0.5)                                       # dy_e = g[group] * v[other end]; D = the group's sum of y * dy; ds = (dy - D) * y * scale
    # by row: dy = 2 2 1 | 2 6, D = 2.5 | 4, ds = -.25 -.25 -.75 | -1 1 (scale 1)
    dq, dq32, dk, _, dv, _ = bw.backward(sub_ptr, sub_col, Q, K, V, G, y, by="row")
    assert dq[:, 0].tolist() == [(-.25 * 16 + -.25 * 16) + -.75 * 8, 0, -1 * 8 + 1 * 32] and not np.signbit(dq[1, 0])   # along: k at the ids, row 1 empty
    assert dk[:, 0].tolist() == [-.75 * 1 + -1 * 4, -.25 * 1 + -.25 * 1, 1 * 4]                                         # across: q at the rows, ascending e
    assert dv[:, 0].tolist() == [.5 * 1 + .5 * 2, .5 * 1 + .5 * 1, .5 * 2] and dq32.dtype == np.float32 and np.array_equal(dq32, dq.astype(np.float32))
    # by column: groups {2,3} {0,1} {4}, g read at the target, v at the row: dy = 0 0 1 3 6, D = 2 | 0 | 3, scale 0.5
    dq, _, dk, _, dv, _ = bw.backward(sub_ptr, sub_col, Q, K, V, G, y, scale=0.5, by="col")
    ds = [0, 0, (1 - 2) * .5 * .5, (3 - 2) * .5 * .5, (6 - 3) * .5 * .5]
    assert dq[:, 0].tolist() == [ds[2] * 8 + ds[3] * 32, ds[0] * 8 + ds[1] * 8, ds[4] * 32]                              # along: k at the rows of the in-edges
    assert dk[:, 0].tolist() == [(ds[0] * 2 + ds[1] * 2) + ds[2] * 1, 0, ds[3] * 1 + ds[4] * 4]                          # across: q at the targets, row order
    assert dv[:, 0].tolist() == [(.5 * 0 + .5 * 0) + .5 * 1, 0, .5 * 1 + .5 * 2]


def test_header_library_and_binding_name_the_call(tmp_path):
    import abi_header
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = abi_header.source(HEADER)
    assert "typedef" not in text and abi_header.structs(text) == {}
    declared = abi_header.prototypes(text, capi.STRUCTS)
    assert list(declared) == [NAME] == capi.EDGE_ATTENTION_BWD_SYMBOLS == list(capi.ABI_EDGE_ATTENTION_BWD)
    raw = open(HEADER).read()
    assert '#include "fora_hip_edge_attention.h"' in raw and "EDGE ATTENTION, BACKWARD" in raw
    lib = capi.load()
    test_only, restype, argtypes = capi.ABI_EDGE_ATTENTION_BWD[NAME]
    assert not test_only and restype is declared[NAME][0] is ctypes.c_int and argtypes == declared[NAME][1] and len(argtypes) == 24
    fn = getattr(lib, NAME)
    assert fn.restype is ctypes.c_int and fn.argtypes == argtypes                    # (load() bound the seventh table too)
    assert len(capi.ABI_EDGE_ATTENTION) == 1 and NAME not in set(capi.ABI) | set(capi.ABI_EXT) | set(capi.ABI_GNN) | set(capi.ABI_EDGE) | set(capi.ABI_EDGE_SOFTMAX)
    x, gr = (ctypes.c_float * 4)(), capi.AttnGrads(lddq=1, lddk=1, lddv=1)
    gr.dq32 = ctypes.addressof(x)
    assert fn(None, x, 0, 1, x, 0, 1, x, 0, 1, x, 0, 1, x, 0, 1, 1, 1, 1, 1.0, 0, ctypes.byref(gr), None, None) == -1   # a NULL ctx: answered without a GPU
    assert list(inspect.signature(capi.Engine.subgraph_attention_bwd).parameters)[:14] == ["self", "Q", "K", "V", "G", "y", "heads", "scale", "by", "want_dq", "want_dk",
                                                                                           "want_dv", "want32", "want64"]
    src = tmp_path / "edge_attention_bwd.c"                                          # the header is plain C99
    src.write_text('#include "fora_hip_edge_attention_bwd.h"\nint main(void) { float x = 0; fora_attn_grads g = {0}; g.dq32 = &x; g.lddq = 1; '
                   'return fora_hip_subgraph_attention_bwd(0, &x, FORA_PROP_F32, 1, &x, FORA_PROP_BF16, 1, &x, FORA_PROP_E4M3, 1, &x, FORA_PROP_F16, 1, &x, FORA_PROP_F64, 1, '
                   '1, 1, 1, 1.0, FORA_SUB_BY_COL, &g, 0, 0) + fora_hip_subgraph_attention(0, &x, 0, 1, &x, 0, 1, &x, 0, 1, 1, 1, 1, 1.0, 0, &x, 0, 1, 0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_torch_function_is_there_with_its_refusals():
    import torch
    from fora_amd import torch_ops as t
    x = torch.zeros((2, 4))
    assert list(inspect.signature(t.subgraph_attention_trained).parameters) == ["engine", "Q", "K", "V", "heads", "scale", "direction"]
    refused = [lambda: t.subgraph_attention_trained(None, x, x, x, heads=3), lambda: t.subgraph_attention_trained(None, x, x, x, heads=0),
               lambda: t.subgraph_attention_trained(None, x, x, x[:, :3], heads=2),                                    # heads divide V's columns too
               lambda: t.subgraph_attention_trained(None, x, x[:, :2], x), lambda: t.subgraph_attention_trained(None, x, x, x, direction="both"),
               lambda: t.subgraph_attention_trained(None, x, x.to(torch.float8_e5m2).requires_grad_(True), x)]         # an FP8 leaf
    for call in refused:
        with pytest.raises(ValueError):
            call()
