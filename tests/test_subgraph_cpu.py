"""The arithmetic of SUBGRAPH (fora_amd/csrc/fora_subgraph_plan.h) checked on the CPU: tests/subgraph_plan_check.cpp restates
rows, count, scan and write on the host through the header's functions, holds them to brute force, and runs under the address
and undefined-behaviour sanitizers.  The sanitized code is that stand-alone program and nothing else.  The numpy twin
(tests/subgraph_ref.py) and the boundary (the extension header, the library, capi.ABI_EXT) are checked here too."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import subgraph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_HEADER = os.path.join(ROOT, "include", "fora_hip_ext.h")
NS = [1, 63, 64, 65, 129, 2000]
SPANS = [256, 1024, 2048]          # the minimum and two larger values
NAMES = ["fora_hip_sparse_subgraph", "fora_hip_sparse_subgraph_fetch"]


@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("subgraph") / "subgraph_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "subgraph_plan_check.cpp")], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    return r.stdout.splitlines()


def _join(xs):
    return ",".join(map(str, xs)) or "-"


def _list(line, dtype):
    return np.zeros(0, dtype) if line == "-" else np.array(line.split(","), dtype=dtype)


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("n", NS)
def test_the_degree_patterns_and_node_sets_every_n_must_survive(plan_check, n, span):
    """all 0, all 1, a hub of 20 spans among rows of 0 and 1, rows that end on a span boundary, leading and trailing empty rows,
    with self-loops and duplicate edges; U empty, single, {0, n - 1}, every node, both sides of each word boundary: inside
    the program"""
    out = _run(plan_check, "all", n, span)[-1].split()
    assert out[-1] == "ok" and int(out[0].split("=")[1]) >= 5 * 7, out


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("n", NS)
def test_random_graphs_against_the_twin(plan_check, n, span):
    rng = np.random.Generator(np.random.PCG64(n * 11 + span))
    deg = rng.integers(0, 4, size=n)
    deg[rng.integers(0, n)] = 700                                  # more than two spans at the minimum, with duplicates
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, n, size=int(row_ptr[-1])).astype(np.int32)
    for count in (1, 5, 64, n):
        cols = np.unique(rng.integers(0, n, size=count)) if count < n else np.arange(n)
        head, *arrays = _run(plan_check, "graph", n, span, _join(row_ptr), _join(col), _join(cols))
        f = {k: int(v) for k, v in (w.split("=") for w in head.split()[:-1])}
        sub_ptr, sub_col, sub_eid, scanned = subgraph_ref.induced(row_ptr, col, cols)
        assert f == {"edges": sub_col.size, "scanned": scanned, "spans": -(-scanned // span)}
        assert np.array_equal(_list(arrays[0], np.int64), sub_ptr)
        assert np.array_equal(_list(arrays[1], np.int32), sub_col) and np.array_equal(_list(arrays[2], np.int64), sub_eid)


def test_span_option_is_a_power_of_two_from_256_to_8192(plan_check):
    got = [int(_run(plan_check, "span", v)[0]) for v in (-5, 0, 1, 255, 256, 257, 511, 512, 1000, 2048, 4095, 4096, 8191, 8192, 8193, 1 << 40)]
    assert got == [256, 256, 256, 256, 256, 256, 256, 512, 512, 2048, 2048, 4096, 4096, 8192, 8192, 8192]


def test_twin_rules():
    # 0 -> 1, 1, 0 (a duplicate edge and a self-loop); 1 -> 2; 2 -> nothing; 3 -> 0, 3
    row_ptr, col = np.array([0, 3, 4, 4, 6]), np.array([1, 1, 0, 2, 0, 3])
    sub_ptr, sub_col, sub_eid, scanned = subgraph_ref.induced(row_ptr, col, [0, 1, 3])
    assert (sub_ptr.dtype, sub_col.dtype, sub_eid.dtype) == (np.int64, np.int32, np.int64)
    assert sub_ptr.tolist() == [0, 3, 3, 5] and sub_col.tolist() == [1, 1, 0, 0, 2] and sub_eid.tolist() == [0, 1, 2, 4, 5]
    assert scanned == 6
    assert (col[sub_eid] == np.array([0, 1, 3])[sub_col]).all()                  # eid names the edge, col the rank of its target
    every = subgraph_ref.induced(row_ptr, col, np.arange(4))                     # every node: the graph itself
    assert every[0].tolist() == row_ptr.tolist() and every[1].tolist() == col.tolist() and every[2].tolist() == list(range(6))
    none = subgraph_ref.induced(row_ptr, col, [])
    assert none[0].tolist() == [0] and none[1].size == 0 and none[2].size == 0 and none[3] == 0
    lone = subgraph_ref.induced(row_ptr, col, [2])                               # a node without out-edges
    assert lone[0].tolist() == [0, 0] and lone[3] == 0


def test_extension_header_library_and_binding_name_the_subgraph():
    import abi_header
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = abi_header.source(EXT_HEADER)
    assert "typedef" not in text and abi_header.structs(text) == {}              # statistics leave through out-pointers
    declared = abi_header.prototypes(text, capi.STRUCTS)
    assert sorted(declared) == sorted(NAMES) == sorted(capi.EXT_SYMBOLS) == sorted(capi.ABI_EXT)
    for name, (restype, argtypes) in declared.items():
        test_only, got_restype, got_argtypes = capi.ABI_EXT[name]
        assert not test_only and got_restype is restype is ctypes.c_int, name
        assert got_argtypes == argtypes, (name, got_argtypes, argtypes)          # (arity and every type)
    # the core tables are what they were
    assert len(capi.ABI) == 68 and len(capi.SYMBOLS) == 63 and not set(NAMES) & set(capi.ABI)
    core = abi_header.source()
    assert not any(name in core for name in NAMES)
    lib = capi.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes == capi.ABI_EXT[name][2], name   # (load() bound the second table too)
    for m in ("sparse_subgraph", "store_take_subgraph"):
        assert callable(getattr(capi.Engine, m))
    assert callable(capi.subgraph_edge_index)
    # a NULL ctx is answered without touching the GPU (there is none here)
    one = (ctypes.c_int64 * 2)()
    assert lib.fora_hip_sparse_subgraph(None, one, 0, one, None, None) == -1
    assert lib.fora_hip_sparse_subgraph_fetch(None, None, None, None, 0) == -1
    with pytest.raises(ctypes.ArgumentError):
        lib.fora_hip_sparse_subgraph_fetch(None, None, None, None, 0.5)
    assert "sub_span" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_extension_header_is_plain_c99(tmp_path):
    src = tmp_path / "ext.c"
    src.write_text('#include "fora_hip_ext.h"\nint main(void) { int64_t e = 0; return fora_hip_sparse_subgraph(0, &e, 0, &e, 0, 0) + fora_hip_sparse_subgraph_fetch(0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_edge_index_of_a_csr():
    from fora_amd import capi
    ei = capi.subgraph_edge_index(np.array([0, 3, 3, 5]), np.array([1, 1, 0, 0, 2], dtype=np.int32))
    assert ei.dtype == np.int64 and ei.tolist() == [[0, 0, 0, 2, 2], [1, 1, 0, 0, 2]]
    assert capi.subgraph_edge_index(np.array([0]), np.zeros(0, np.int32)).shape == (2, 0)
