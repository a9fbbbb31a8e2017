"""EDGE GAT and EDGE GAT, BACKWARD (include/fora_hip_edge_gat.h) checked on the CPU: the numpy twin (tests/subgraph_gat_ref.py) by
hand and against a plain float64 formula, and the boundary -- the eighth header, the library, capi.ABI_EDGE_GAT, the Engine methods
and the torch function."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import subgraph_gat_ref as gat
import subgraph_prop_ref as sr
import subgraph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fora_hip_edge_gat.h")
NAMES = ["fora_hip_subgraph_gat", "fora_hip_subgraph_gat_bwd"]


def test_twin_by_hand():
    # the four-node graph of test_subgraph_attention_cpu: the edges (0,1) (0,1) (0,0) (2,0) (2,2) -- rows {0,1,2} {} {3,4}, columns {2,3} {0,1} {4}
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(np.array([0, 3, 4, 4, 6]), np.array([1, 1, 0, 2, 0, 3]), [0, 1, 3])
    f = lambda *x: np.array(x, dtype=np.float32).reshape(-1, 1)
    el, er, V, G, third = f(1, 7, -3), f(1, 1, -2000), f(1, 2, 4), f(1, 0, 2), 1.0 / 3.0
    # z = el[row] + er[col] = 2 2 2 -2 -2003 whichever the grouping; slope .5: s = 2 2 2 -1 -1001.5
    assert gat.pre_activation(sub_ptr, sub_col, el, er).tolist() == [[2, 2, 2, -2, -2003]]
    out, out32, y, _, nan = gat.forward(sub_ptr, sub_col, el, er, V, slope=0.5, by="row")     # rows: equal scores; exp(-1000.5) is 0
    assert y.tolist() == [[third, third, third, 1, 0]] and nan == 0 and np.array_equal(out32, out.astype(np.float32))
    assert out[:, 0].tolist() == [(third * 2 + third * 2) + third * 1, 0, 1 * 1 + 0 * 4] and not np.signbit(out[1, 0])      # v at the targets; row 1 empty
    out, _, y, _, _ = gat.forward(sub_ptr, sub_col, f(1, 7, 1), f(1, 1, 5), V, slope=0.5, by="col")   # z = 2 2 2 2 6: columns of equal scores
    assert y.tolist() == [[.5, .5, .5, .5, 1]] and out[:, 0].tolist() == [.5 * 1 + .5 * 4, .5 * 1 + .5 * 1, 1 * 4]        # v at the rows, ascending e
    # backward on y = .5: dy_e = g[group] * v[other end], D = the group's sum of y * dy, ds = (dy - D) * y, dz = ds where z >= 0, else ds * .5
    y = np.full((1, 5), 0.5)
    # by row: dy = 2 2 1 | 2 8, D = 2.5 | 5, ds = -.25 -.25 -.75 | -1.5 1.5, dz = -.25 -.25 -.75 | -.75 .75
    dl, dl32, dr, _, dv, _ = gat.backward(sub_ptr, sub_col, el, er, V, G, y, slope=0.5, by="row")
    assert dl[:, 0].tolist() == [(-.25 + -.25) + -.75, 0, -.75 + .75] and dl32.dtype == np.float32                          # along: the rows
    assert dr[:, 0].tolist() == [-.75 + -.75, -.25 + -.25, .75] and dv[:, 0].tolist() == [.5 * 1 + .5 * 2, .5 * 1 + .5 * 1, .5 * 2]   # across: the columns
    # by column: dy = v[row] * g[col] = 0 0 1 4 8, D = 2.5 | 0 | 4, ds = 0 0 -.75 .75 2, dz = 0 0 -.75 .375 1
    dl, _, dr, _, dv, _ = gat.backward(sub_ptr, sub_col, el, er, V, G, y, slope=0.5, by="col")
    assert dr[:, 0].tolist() == [-.75 + .375, 0, 1] and dl[:, 0].tolist() == [(0 + 0) + -.75, 0, .375 + 1]                 # er is the group's operand now
    assert dv[:, 0].tolist() == [(.5 * 0 + .5 * 0) + .5 * 1, 0, .5 * 1 + .5 * 2]


@pytest.mark.parametrize("by", ["row", "col"])
def test_twin_against_a_plain_formula(by):
    """the twin and np.exp with ordinary sums differ in the order of the sums and in exp_def's documented 1 ulp: with L the group's
    length, |twin - plain| <= (2 L + 32) * 2^-53 * sum_e |y_e v_e| per output -- L rounding steps in each of the two sums (the
    softmax's and the product's), and a few ulps per term for exp, the division and the product"""
    row_ptr, col, U = sr.crafted_graph()
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(row_ptr, col, U)
    heads, dv, slope, nc = 2, 3, 0.2, U.size
    rng = np.random.Generator(np.random.PCG64(10500))
    el, er, V = (rng.standard_normal((nc, w)).astype(np.float32) for w in (heads, heads, heads * dv))
    out = gat.forward(sub_ptr, sub_col, el, er, V, heads=heads, slope=slope, by=by)[0]
    rows, cols = np.repeat(np.arange(nc), np.diff(sub_ptr)), np.asarray(sub_col, dtype=np.int64)
    group, other = (rows, cols) if by == "row" else (cols, rows)
    z = el.astype(np.float64)[rows] + er.astype(np.float64)[cols]
    s = np.where(z >= 0, z, z * slope)                                                       # [edges, heads]
    worst = 0.0
    for j in range(nc):
        e = np.flatnonzero(group == j)
        if not e.size:
            assert not out[j].any()
            continue
        p = np.exp(s[e] - s[e].max(axis=0))
        terms = np.repeat(p / p.sum(axis=0), dv, axis=1) * V.astype(np.float64)[other[e]]     # [L, heads * dv]
        bound = (2 * e.size + 32) * 2.0 ** -53 * np.abs(terms).sum(axis=0)
        err = np.abs(out[j] - terms.sum(axis=0))
        assert (err <= bound).all(), (j, e.size)
        worst = max(worst, float((err / bound).max()))
    print(f"largest |twin - plain| / bound by {by}: {worst:.3f}")


def test_header_library_and_binding_name_the_calls(tmp_path):
    import abi_header
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = abi_header.source(HEADER)
    assert "typedef" not in text and abi_header.structs(text) == {}
    declared = abi_header.prototypes(text, capi.STRUCTS)
    assert list(declared) == NAMES == capi.EDGE_GAT_SYMBOLS == list(capi.ABI_EDGE_GAT)
    raw = open(HEADER).read()
    assert '#include "fora_hip_edge_attention_bwd.h"' in raw and "EDGE GAT, BACKWARD" in raw
    lib = capi.load()
    for name, nargs in zip(NAMES, (22, 23)):
        test_only, restype, argtypes = capi.ABI_EDGE_GAT[name]
        assert not test_only and restype is declared[name][0] is ctypes.c_int and argtypes == declared[name][1] and len(argtypes) == nargs
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes == argtypes                # (load() bound the eighth table too)
        assert name not in set(capi.ABI) | set(capi.ABI_EXT) | set(capi.ABI_GNN) | set(capi.ABI_EDGE) | set(capi.ABI_EDGE_SOFTMAX) | set(capi.ABI_EDGE_ATTENTION) | set(capi.ABI_EDGE_ATTENTION_BWD)
    x, gr = (ctypes.c_float * 4)(), capi.AttnGrads(lddq=1, lddk=1, lddv=1)
    gr.dq32 = ctypes.addressof(x)
    assert lib.fora_hip_subgraph_gat(None, x, 0, 1, x, 0, 1, x, 0, 1, 1, 1, 0.2, 0, x, None, 1, None, None, 0, None, None) == -1   # a NULL ctx: answered without a GPU
    assert lib.fora_hip_subgraph_gat_bwd(None, x, 0, 1, x, 0, 1, x, 0, 1, x, 0, 1, x, 0, 1, 1, 1, 0.2, 0, ctypes.byref(gr), None, None) == -1
    assert list(inspect.signature(capi.Engine.subgraph_gat).parameters)[:11] == ["self", "el", "er", "V", "heads", "slope", "by", "want32", "want64", "want_y32", "want_y64"]
    assert list(inspect.signature(capi.Engine.subgraph_gat_bwd).parameters)[:14] == ["self", "el", "er", "V", "G", "y", "heads", "slope", "by", "want_del", "want_der", "want_dv",
                                                                                     "want32", "want64"]
    src = tmp_path / "edge_gat.c"                                                    # the header is plain C99
    src.write_text('#include "fora_hip_edge_gat.h"\nint main(void) { float x = 0; fora_attn_grads g = {0}; g.dq32 = &x; g.lddq = 1; '
                   'return fora_hip_subgraph_gat(0, &x, FORA_PROP_F32, 1, &x, FORA_PROP_BF16, 1, &x, FORA_PROP_E4M3, 1, 1, 1, 0.2, FORA_SUB_BY_COL, &x, 0, 1, 0, 0, 0, 0, 0) + '
                   'fora_hip_subgraph_gat_bwd(0, &x, FORA_PROP_F32, 1, &x, FORA_PROP_F16, 1, &x, FORA_PROP_E5M2, 1, &x, FORA_PROP_BF16, 1, &x, FORA_PROP_F64, 1, 1, 1, 0.2, 0, &g, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_torch_function_is_there_with_its_refusals():
    import torch
    from fora_amd import torch_ops as t
    e, x = torch.zeros((2, 2)), torch.zeros((2, 4))
    assert list(inspect.signature(t.subgraph_gat).parameters) == ["engine", "el", "er", "V", "heads", "slope", "direction"]
    assert [p.default for p in inspect.signature(t.subgraph_gat).parameters.values()][4:] == [1, 0.2, "out"]
    refused = [lambda: t.subgraph_gat(None, e, e, x, heads=1), lambda: t.subgraph_gat(None, e, e, x, heads=0),                 # el and er are [nc, heads]
               lambda: t.subgraph_gat(None, e, e, x[:, :3], heads=2), lambda: t.subgraph_gat(None, e, e[:, :1], x, heads=2),
               lambda: t.subgraph_gat(None, e, e, x, heads=2, direction="both"),
               lambda: t.subgraph_gat(None, e, e.to(torch.float8_e5m2).requires_grad_(True), x, heads=2)]                       # an FP8 leaf
    for call in refused:
        with pytest.raises(ValueError):
            call()
