"""SUBGRAPH PRODUCTS (include/fora_hip_gnn.h) checked on the CPU: the numpy twin (tests/subgraph_prop_ref.py) by hand; the host
side (fora_amd/csrc/fora_subgraph_prop_plan.h: the option's clamp, the split into the one-pass kernel's rows and the long
path's, the long path's plan, the transposition) through tests/subgraph_prop_plan_check.cpp, which holds it to brute force under
the address and undefined-behaviour sanitizers -- that stand-alone program is the only sanitized code; and the boundary: the
third header, the library, capi.ABI_GNN, the Engine methods and the torch operation."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import subgraph_prop_ref as sr
import subgraph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GNN_HEADER = os.path.join(ROOT, "include", "fora_hip_gnn.h")
NAMES = ["fora_hip_subgraph_propagate", "fora_hip_subgraph_propagate_t", "fora_hip_subgraph_transpose_fetch"]
EXT_NAMES = ["fora_hip_sparse_subgraph", "fora_hip_sparse_subgraph_fetch"]
LENS = [0, 1, 63, 64, 65, 255, 256, 257, 300, 700]
SHORTS = [0, 64, 256]


@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("subgraph_prop") / "subgraph_prop_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "subgraph_prop_plan_check.cpp")], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    return r.stdout.splitlines()


def _join(xs):
    return ",".join(map(str, xs)) or "-"


def _list(line, dtype):
    return np.zeros(0, dtype) if line == "-" else np.array(line.split(","), dtype=dtype)


def test_twin_by_hand():
    # the four-node graph of test_subgraph_cpu.test_twin_rules: 0 -> 1, 1, 0; 1 -> 2; 2 -> nothing; 3 -> 0, 3; U = {0, 1, 3}
    row_ptr, col = np.array([0, 3, 4, 4, 6]), np.array([1, 1, 0, 2, 0, 3])
    sub_ptr, sub_col, _, _ = subgraph_ref.induced(row_ptr, col, [0, 1, 3])
    assert sub_ptr.tolist() == [0, 3, 3, 5] and sub_col.tolist() == [1, 1, 0, 0, 2]
    X = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]], dtype=np.float32)          # rows of local nodes 0, 1, 2
    out64, out32 = sr.propagate(sub_ptr, sub_col, X)
    # row 0: x1 + x1 + x0 (the duplicate edge counts twice, the self-loop once); row 1: no edge inside U; row 2: x0 + x2
    assert out64.tolist() == [[5.0, 50.0], [0.0, 0.0], [5.0, 50.0]] and out32.dtype == np.float32 and out64.dtype == np.float64
    assert not np.signbit(out64[1]).any()                                              # a row without terms is +0.0
    t64, _ = sr.propagate_t(sub_ptr, sub_col, X)
    # column 0: rows 0 and 2; column 1: row 0 twice; column 2: row 2
    assert t64.tolist() == [[5.0, 50.0], [2.0, 20.0], [4.0, 40.0]]
    m64, m32 = sr.propagate(sub_ptr, sub_col, X, mean=True)
    assert m64.tolist() == [[5.0 / 3.0, 50.0 / 3.0], [0.0, 0.0], [2.5, 25.0]] and (m32 == m64.astype(np.float32)).all()
    mt64, _ = sr.propagate_t(sub_ptr, sub_col, X, mean=True)
    assert mt64.tolist() == [[2.5, 25.0], [1.0, 10.0], [4.0, 40.0]]
    w = np.array([0.5, 0.25, 2.0, 3.0, -1.0], dtype=np.float32)                       # one per edge, in the order of sub_col
    v64, _ = sr.propagate(sub_ptr, sub_col, X, values=w)
    assert v64.tolist() == [[0.5 * 2 + 0.25 * 2 + 2.0 * 1, 0.5 * 20 + 0.25 * 20 + 2.0 * 10], [0.0, 0.0], [3.0 * 1 - 4.0, 3.0 * 10 - 40.0]]
    vt64, _ = sr.propagate_t(sub_ptr, sub_col, X, values=w)                            # values stay indexed by the edge's place
    assert vt64.tolist() == [[2.0 * 1 + 3.0 * 4, 2.0 * 10 + 3.0 * 40], [0.5 * 1 + 0.25 * 1, 0.5 * 10 + 0.25 * 10], [-4.0, -40.0]]
    in_ptr, in_row, in_pos = sr.transpose(sub_ptr, sub_col)
    assert (in_ptr.dtype, in_row.dtype, in_pos.dtype) == (np.int64, np.int32, np.int64)
    assert in_ptr.tolist() == [0, 2, 4, 5] and in_row.tolist() == [0, 2, 0, 0, 2] and in_pos.tolist() == [2, 3, 0, 1, 4]
    # a column without edges: U = {0, 3} drops node 1 -- column... every column of this one has an edge, row 1 of the other has none
    lone = subgraph_ref.induced(row_ptr, col, [1, 2])                                  # 1 -> 2 only: row 1 and column 0 are empty
    l64, _ = sr.propagate_t(lone[0], lone[1], X[:2], mean=True)
    assert l64.tolist() == [[0.0, 0.0], [1.0, 10.0]] and not np.signbit(l64[0]).any()
    assert sr.mean_backward_operand(np.array([[3.0], [5.0]], np.float32), [3, 0]).tolist() == [[1.0], [5.0]]


def test_the_order_of_the_additions_is_the_contract():
    # 300 terms whose sum depends on the order and on the cut at 256: the twin's segments are the contract's
    rng = np.random.Generator(np.random.PCG64(5))
    X = np.ldexp(rng.standard_normal((300, 1)), rng.integers(-20, 21, size=(300, 1))).astype(np.float32)
    sub_ptr = np.concatenate([[0, 300], np.full(299, 300)]).astype(np.int64)
    sub_col = np.arange(300, dtype=np.int32)
    out64, _ = sr.propagate(sub_ptr, sub_col, X)
    p0 = p1 = 0.0
    for e in range(256):
        p0 = p0 + float(X[e, 0])
    for e in range(256, 300):
        p1 = p1 + float(X[e, 0])
    assert out64[0, 0] == p0 + p1


@pytest.mark.parametrize("segs", [1, 3, 1000])
@pytest.mark.parametrize("short", SHORTS)
def test_crafted_lengths_and_empty_cases_against_brute_force(plan_check, short, segs):
    """rows and columns of 0, 1, 63, 64, 65, 255, 256, 257, 300 and 700 edges, a duplicate edge, a self-loop, empty leading and
    trailing rows; no rows; rows without edges: inside the program"""
    out = _run(plan_check, "all", short, segs)[-1].split()
    assert out[-1] == "ok" and int(out[0].split("=")[1]) >= 5, out


@pytest.mark.parametrize("short", SHORTS)
def test_random_subgraphs_against_the_twin(plan_check, short):
    rng = np.random.Generator(np.random.PCG64(short + 17))
    nc = 400
    deg = rng.integers(0, 4, size=nc)
    deg[[5, 6, 7, 8, 9, 10, 11, 12, 13]] = LENS[1:]                     # the lengths as rows; targets drawn with duplicates
    deg[0] = deg[-1] = 0
    sub_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    sub_col = rng.integers(0, nc, size=int(sub_ptr[-1])).astype(np.int32)
    sub_col[rng.integers(0, sub_col.size, size=700)] = 3                # a hub column
    sub_col[sub_ptr[20]:sub_ptr[21]] = 20                               # self-loops
    head, *arrays = _run(plan_check, "csr", short, 2, _join(sub_ptr), _join(sub_col))
    f = {k: int(v) for k, v in (w.split("=") for w in head.split()[:-1])}
    in_ptr, in_row, in_pos = sr.transpose(sub_ptr, sub_col)
    lens, tlens = np.diff(sub_ptr), np.diff(in_ptr)
    assert f == {"short": int((lens <= short).sum()), "long": int((lens > short).sum()), "segs": int(((lens[lens > short] + 255) // 256).sum()),
                 "chunks": max(1, -(-int(((lens[lens > short] + 255) // 256).sum()) // 2)),
                 "t_short": int((tlens <= short).sum()), "t_long": int((tlens > short).sum()), "t_segs": int(((tlens[tlens > short] + 255) // 256).sum())}
    assert np.array_equal(_list(arrays[0], np.int64), in_ptr)
    assert np.array_equal(_list(arrays[1], np.int32), in_row) and np.array_equal(_list(arrays[2], np.int64), in_pos)


def test_sub_short_is_clamped_to_0_256(plan_check):
    got = [int(_run(plan_check, "cap", v)[0]) for v in (-(1 << 40), -1, 0, 1, 64, 255, 256, 257, 1000, 1 << 40)]
    assert got == [0, 0, 0, 1, 64, 255, 256, 256, 256, 256]


def test_gnn_header_library_and_binding_name_the_subgraph_products():
    import abi_header
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = abi_header.source(GNN_HEADER)
    assert "typedef" not in text and abi_header.structs(text) == {}              # statistics leave through out-pointers
    declared = abi_header.prototypes(text, capi.STRUCTS)
    assert sorted(declared) == sorted(NAMES) == sorted(capi.GNN_SYMBOLS) == sorted(capi.ABI_GNN)
    for name, (restype, argtypes) in declared.items():
        test_only, got_restype, got_argtypes = capi.ABI_GNN[name]
        assert not test_only and got_restype is restype is ctypes.c_int, name
        assert got_argtypes == argtypes, (name, got_argtypes, argtypes)          # (arity and every type)
    assert '#include "fora_hip_ext.h"' in open(GNN_HEADER).read() and "SUBGRAPH PRODUCTS" in open(GNN_HEADER).read()
    assert capi.SUB_MEAN == 1 and "#define FORA_SUB_MEAN 1" in open(GNN_HEADER).read()
    # the two older censuses are what they were
    assert len(capi.ABI) == 68 and len(capi.SYMBOLS) == 63 and sorted(capi.ABI_EXT) == sorted(capi.EXT_SYMBOLS) == sorted(EXT_NAMES)
    assert not set(NAMES) & (set(capi.ABI) | set(capi.ABI_EXT))
    core, ext = abi_header.source(), abi_header.source(os.path.join(ROOT, "include", "fora_hip_ext.h"))
    assert not any(name in core or name in ext for name in NAMES)
    assert sorted(abi_header.prototypes(ext, capi.STRUCTS)) == sorted(EXT_NAMES)
    lib = capi.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes == capi.ABI_GNN[name][2], name   # (load() bound the third table too)
    for m in ("subgraph_propagate", "subgraph_propagate_t", "subgraph_transpose_fetch"):
        assert callable(getattr(capi.Engine, m))
    # a NULL ctx is answered without touching the GPU (there is none here)
    x = (ctypes.c_float * 4)()
    assert lib.fora_hip_subgraph_propagate(None, x, 0, 1, 1, 0, None, 0, x, None, 1, None, None) == -1
    assert lib.fora_hip_subgraph_propagate_t(None, x, 0, 1, 1, 0, None, 0, x, None, 1, None, None) == -1
    assert lib.fora_hip_subgraph_transpose_fetch(None, None, None, None, 0) == -1
    with pytest.raises(ctypes.ArgumentError):
        lib.fora_hip_subgraph_transpose_fetch(None, None, None, None, 0.5)
    assert "sub_short" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_torch_operation_is_there():
    import inspect
    import torch
    from fora_amd import torch_ops
    x = torch.zeros((2, 2))
    with pytest.raises(ValueError):                                                    # values that require grad: refused before anything runs
        torch_ops.subgraph_propagate(None, x, values=torch.zeros(3, requires_grad=True))
    with pytest.raises(ValueError):
        torch_ops.subgraph_propagate(None, x, direction="both")
    with pytest.raises(ValueError):
        torch_ops.subgraph_propagate(None, x, values=torch.zeros(3), norm="mean")
    with pytest.raises(ValueError):
        torch_ops.subgraph_propagate(None, x.to(torch.float8_e4m3fn).requires_grad_(True))
    assert list(inspect.signature(torch_ops.subgraph_propagate).parameters) == ["engine", "X", "values", "norm", "direction"]
    assert issubclass(torch_ops._SubgraphPropagate, torch_ops.torch.autograd.Function)
    assert "float32(float64(G[j]) / float64(count_j))" in torch_ops.subgraph_propagate.__doc__   # the stated composition


def test_the_gnn_header_is_plain_c99(tmp_path):
    src = tmp_path / "gnn.c"
    src.write_text('#include "fora_hip_gnn.h"\nint main(void) { float x = 0; return fora_hip_subgraph_propagate(0, &x, FORA_PROP_F32, 1, 1, FORA_SUB_MEAN, 0, 0, &x, 0, 1, 0, 0)'
                   ' + fora_hip_subgraph_propagate_t(0, &x, 0, 1, 1, 0, 0, 0, &x, 0, 1, 0, 0) + fora_hip_subgraph_transpose_fetch(0, 0, 0, 0, 0)'
                   ' + fora_hip_sparse_subgraph_fetch(0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
