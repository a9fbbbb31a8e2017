"""SUBGRAPH POOL (include/fora_hip_pool.h) checked on the CPU: the numpy twin (tests/subgraph_pool_ref.py) by hand, and the boundary
-- the ninth header, the library, capi.ABI_POOL, the Engine methods and the torch function."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import subgraph_pool_ref as pool
import subgraph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fora_hip_pool.h")
NAMES = ["fora_hip_subgraph_pool", "fora_hip_subgraph_pool_bwd"]
NAN = float("nan")
# the four-node graph of test_subgraph_cpu.test_twin_rules: the edges e0 e1 (0,1) e2 (0,0) e3 (2,0) e4 (2,2) -- rows {0,1,2} {} {3,4} read
# the nodes (1,1,0) () (0,2); columns {2,3} {0,1} {4} read (0,2) (0,0) (2).  X by column: a tie of the extremes; both zeros; a NaN
X = np.array([[3, 0.0, NAN], [7, -0.0, 4], [7, -0.0, 9]], dtype=np.float32)
HAND = {  # (by, op): the value and the edge of every (node, column); -0.0 and +0.0 as written, row 1 is empty
    ("row", "max"): ([[7, -0.0, NAN], [0, 0, 0], [7, 0.0, NAN]], [[0, 0, 2], [-1, -1, -1], [4, 3, 3]]),
    ("row", "min"): ([[3, -0.0, NAN], [0, 0, 0], [3, 0.0, NAN]], [[2, 0, 2], [-1, -1, -1], [3, 3, 3]]),
    ("col", "max"): ([[7, 0.0, NAN], [3, 0.0, NAN], [7, -0.0, 9]], [[3, 2, 2], [0, 0, 0], [4, 4, 4]]),
    ("col", "min"): ([[3, 0.0, NAN], [3, 0.0, NAN], [7, -0.0, 9]], [[2, 2, 2], [0, 0, 0], [4, 4, 4]]),
}


@pytest.mark.parametrize("by,op", list(HAND))
def test_twin_by_hand(by, op):
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(np.array([0, 3, 4, 4, 6]), np.array([1, 1, 0, 2, 0, 3]), [0, 1, 3])
    assert sub_ptr.tolist() == [0, 3, 3, 5] and sub_col.tolist() == [1, 1, 0, 0, 2]
    out64, out32, arg = pool.forward(sub_ptr, sub_col, X, op=op, by=by)
    value, edge = HAND[by, op]
    want = np.array(value, dtype=np.float64)
    want[np.isnan(want)] = pool.QNAN
    assert np.array_equal(out64.view(np.uint64), want.view(np.uint64))             # bits: the sign of a zero, the one quiet NaN
    assert np.array_equal(out32.view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert arg.dtype == np.int32 and arg.tolist() == edge
    # backward: the gradient of (j, c) goes to the source of the one edge arg names, added in ascending e
    G = np.array([[1, 2, 3], [10, 20, 30], [100, 200, 300]], dtype=np.float32)
    hand = {("row", "max"): [[0, 200, 3 + 300], [1, 2, 0], [100, 0, 0]], ("col", "max"): [[10, 20 + 2, 30 + 3], [0, 0, 0], [1 + 100, 200, 300]]}
    if (by, op) in hand:
        d64, d32 = pool.backward(sub_ptr, sub_col, G, arg, by=by)
        assert d64.tolist() == hand[by, op] and d32.dtype == np.float32 and d32.tolist() == hand[by, op]
        stale = np.array([[3, 4, -1], [0, 1, 2], [0, 1, 2]] if by == "row" else [[0, 1, 4], [2, 3, -1], [0, 3, 2]], dtype=np.int32)
        assert not pool.backward(sub_ptr, sub_col, G, stale, by=by)[0].any()         # edges of other groups, and none: nothing is added


def test_header_library_and_binding_name_the_calls(tmp_path):
    import abi_header
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = abi_header.source(HEADER)
    assert "typedef" not in text and abi_header.structs(text) == {}
    declared = abi_header.prototypes(text, capi.STRUCTS)
    assert list(declared) == NAMES == capi.POOL_SYMBOLS == list(capi.ABI_POOL)
    raw = open(HEADER).read()
    assert '#include "fora_hip_edge_softmax.h"' in raw and "SUBGRAPH POOL" in raw and capi.POOL_MIN == 4 and "#define FORA_POOL_MIN 4" in raw
    lib = capi.load()
    older = (capi.ABI, capi.ABI_EXT, capi.ABI_GNN, capi.ABI_EDGE, capi.ABI_EDGE_SOFTMAX, capi.ABI_EDGE_ATTENTION, capi.ABI_EDGE_ATTENTION_BWD, capi.ABI_EDGE_GAT)
    for name in NAMES:
        test_only, restype, argtypes = capi.ABI_POOL[name]
        assert not test_only and restype is declared[name][0] is ctypes.c_int and argtypes == declared[name][1] and len(argtypes) == 13
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes == argtypes                # (load() bound the ninth table too)
        assert not any(name in table for table in older)
    x, a = (ctypes.c_float * 4)(), (ctypes.c_int32 * 4)()
    assert lib.fora_hip_subgraph_pool(None, x, 0, 1, 1, 0, x, None, 1, a, 1, None, None) == -1        # a NULL ctx: answered without a GPU
    assert lib.fora_hip_subgraph_pool_bwd(None, x, 0, 1, 1, 0, a, 1, x, None, 1, None, None) == -1
    assert list(inspect.signature(capi.Engine.subgraph_pool).parameters) == ["self", "X", "op", "by", "want32", "want64", "want_arg", "out32", "out64", "arg", "bf16"]
    assert list(inspect.signature(capi.Engine.subgraph_pool_bwd).parameters) == ["self", "G", "arg", "by", "want32", "want64", "out32", "out64", "bf16"]
    src = tmp_path / "pool.c"                                                        # the header is plain C99
    src.write_text('#include "fora_hip_pool.h"\nint main(void) { float x = 0; int32_t a = 0; '
                   'return fora_hip_subgraph_pool(0, &x, FORA_PROP_BF16, 1, 1, FORA_SUB_BY_COL | FORA_POOL_MIN, &x, 0, 1, &a, 1, 0, 0) + '
                   'fora_hip_subgraph_pool_bwd(0, &x, FORA_PROP_F32, 1, 1, 0, &a, 1, &x, 0, 1, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_torch_function_is_there_with_its_refusals():
    import torch
    from fora_amd import torch_ops as t
    assert list(inspect.signature(t.subgraph_pool).parameters) == ["engine", "X", "op", "direction"]
    assert [p.default for p in inspect.signature(t.subgraph_pool).parameters.values()][2:] == ["max", "out"]
    assert "first" in t.subgraph_pool.__doc__ and "scatter_reduce" in t.subgraph_pool.__doc__
    x = torch.zeros((2, 4))
    for call in (lambda: t.subgraph_pool(None, x, op="mean"), lambda: t.subgraph_pool(None, x, direction="both"),
                 lambda: t.subgraph_pool(None, x.to(torch.float8_e5m2).requires_grad_(True))):            # an FP8 leaf
        with pytest.raises(ValueError):
            call()
