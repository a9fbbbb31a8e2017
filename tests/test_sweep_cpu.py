"""The SWEEP CUT contract (include/fora_hip.h) on the CPU: tests/sweep_ref.py, the Python twin the GPU tests compare with,
against a brute force over set membership; the cases without a best prefix; the tie rule; the recovery of a planted block on
rows of the oracle's twin; and the C ABI's new symbols and structs."""
import ctypes
import os
import re

import numpy as np
import pytest

import sweep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX_ONE = 1 << 62


def _random_graph(rng, n, dup=True):
    """directed, with duplicate edges and dangling nodes, no self loops"""
    deg = rng.integers(0, 7, size=n)
    deg[rng.choice(n, size=max(1, n // 6), replace=False)] = 0
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=row_ptr[1:])
    col = np.zeros(int(row_ptr[-1]), dtype=np.int32)
    for u in range(n):
        t = rng.integers(0, n - 1, size=deg[u])
        t = t + (t >= u)  # no self loop
        if dup and deg[u] >= 2:
            t[1] = t[0]   # a stored duplicate
        col[row_ptr[u]:row_ptr[u + 1]] = t
    return row_ptr, col


def _random_row(rng, n, row_ptr):
    """a sparse row with equal keys on several ids: words of the form q * max(deg, 1) (+ a remainder below deg)"""
    deg = np.maximum(np.diff(row_ptr), 1)
    row = np.zeros(n, dtype=np.uint64)
    on = rng.random(n) < 0.6
    q = rng.integers(1, 6, size=n).astype(np.uint64) << np.uint64(40)   # few distinct quotients: ties by id
    rem = rng.integers(0, 1 << 20, size=n).astype(np.uint64) % deg.astype(np.uint64)
    row[on] = (q * deg.astype(np.uint64) + rem)[on]
    return row


def _same(a, b):
    for k in ("len", "order", "cut", "vol", "best", "cut_best", "vol_best", "den"):
        assert a[k] == b[k], k
    assert R.f64_bits(a["conductance"]) == R.f64_bits(b["conductance"])


@pytest.mark.parametrize("seed", range(6))
def test_twin_equals_brute_force(seed):
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    n = int(rng.integers(30, 201))
    row_ptr, col = _random_graph(rng, n)
    deg = np.diff(row_ptr)
    assert (deg == 0).any() and any(col[row_ptr[u]] == col[row_ptr[u] + 1] for u in range(n) if deg[u] >= 2)
    for _ in range(3):
        row = _random_row(rng, n, row_ptr)
        full = R.sweep_row(row, row_ptr, col, 1)
        keys = [int(row[v]) // max(int(deg[v]), 1) for v in full["order"]]
        assert keys == sorted(keys, reverse=True) and len(set(keys)) < len(keys)          # equal keys ...
        assert all(a < b for a, b, ka, kb in zip(full["order"], full["order"][1:], keys, keys[1:]) if ka == kb)  # ... tie by id
        assert (row[full["order"]] > 0).all() and full["len"] == int((row > 0).sum())
        for thr in (1, 3 << 40):
            for max_size in (0, 1, full["len"] // 2, full["len"] + 5):
                a = R.sweep_row(row, row_ptr, col, thr, max_size)
                _same(a, R.sweep_brute(row, row_ptr, col, thr, max_size))
                assert len(a["order"]) == (a["len"] if max_size <= 0 else min(a["len"], max_size))
                assert a["order"] == R.sweep_row(row, row_ptr, col, thr)["order"][:len(a["order"])]


def test_rows_without_a_best_prefix():
    # 0 -> 1, 1 -> 0, 0 -> 2 ; 2 and 3 dangling
    row_ptr = np.array([0, 2, 3, 3, 3], dtype=np.int64)
    col = np.array([1, 2, 0], dtype=np.int32)
    none = dict(best=0, cut_best=0, vol_best=0, den=0, conductance=1.0)

    def check(r, length):
        assert r["len"] == length
        for k, v in none.items():
            assert r[k] == v, k

    check(R.sweep_row(np.zeros(4, dtype=np.uint64), row_ptr, col, 1), 0)                        # an empty row
    check(R.dangling_row(2), 1)                                                                # a dangling source
    r = R.sweep_row(np.array([0, 0, 5, 9], dtype=np.uint64), row_ptr, col, 1)                  # dangling nodes only
    check(r, 2)
    assert r["order"] == [3, 2] and r["cut"] == [0, 0] and r["vol"] == [0, 0]
    # vol == nnz: one node holds every edge
    row_ptr1 = np.array([0, 2, 2, 2], dtype=np.int64)
    col1 = np.array([1, 2], dtype=np.int32)
    r = R.sweep_row(np.array([8, 0, 0], dtype=np.uint64), row_ptr1, col1, 1)
    check(r, 1)
    assert r["cut"] == [2] and r["vol"] == [2]
    # ... while a row over the first graph that reaches vol == nnz only at its end has a best prefix before it
    r = R.sweep_row(np.array([8, 8, 1, 0], dtype=np.uint64), row_ptr, col, 1)
    assert r["order"] == [1, 0, 2] and r["vol"] == [1, 3, 3] and r["cut"] == [1, 1, 0] and (r["best"], r["cut_best"], r["den"]) == (1, 1, 1)


def test_conductance_ties_go_to_the_smaller_prefix():
    # two disjoint 2-cycles {0, 1}, {2, 3} and a tail: the prefixes {0, 1} and {0, 1, 2, 3} both have cut 0
    src = [0, 1, 2, 3, 4, 5]
    dst = [1, 0, 3, 2, 5, 4]
    row_ptr = np.arange(7, dtype=np.int64)
    col = np.array(dst, dtype=np.int32)
    assert src == list(range(6))
    r = R.sweep_row(np.array([60, 50, 40, 30, 0, 0], dtype=np.uint64), row_ptr, col, 1)
    assert r["order"] == [0, 1, 2, 3] and r["cut"] == [1, 0, 1, 0] and r["vol"] == [1, 2, 3, 4]
    assert r["best"] == 2 and r["conductance"] == 0.0
    # cut / den 1/1 at the first prefix and 3/3 at the second
    row_ptr = np.array([0, 1, 3, 5, 6, 7, 8, 9], dtype=np.int64)
    col = np.array([2, 3, 4, 0, 1, 5, 6, 3, 4], dtype=np.int32)
    r = R.sweep_row(np.array([9, 8, 0, 0, 0, 0, 0], dtype=np.uint64), row_ptr, col, 1)
    assert r["cut"] == [1, 3] and r["vol"] == [1, 3] and r["best"] == 1 and r["conductance"] == 1.0


def test_planted_block_is_recovered_on_twin_rows(oracle):
    n, row_ptr, col, block = R.planted_graph()
    assert n == 1999 and block.size == 300
    g = oracle.Graph(n, int(row_ptr[-1]), row_ptr, col)
    rmax, omega = oracle.fora_setting(g.n, g.m, 0.5)
    inside = set(block.tolist())
    rng = np.random.Generator(np.random.PCG64(7100))
    for s in rng.choice(block, size=4, replace=False):
        row, _, _ = oracle.twin_query(g, int(s), rmax, omega, seed=0x464F5241)
        for t in (0.0, 1.0 / n):
            r = R.sweep_row(row, row_ptr, col, R.thr_fix_of(t))
            got = set(r["order"][:r["best"]])
            jac = len(got & inside) / len(got | inside)
            print(f"source {int(s)} threshold {t:g}: best {r['best']} conductance {r['conductance']:.4f} jaccard {jac:.4f}")
            assert jac >= 0.9, (int(s), t, jac)


def test_c_abi_declares_exports_and_binds_the_sweep():
    hdr = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("fora_hip_sweep_batch", "fora_hip_sweep_fetch", "fora_hip_sweep_clear"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    assert "SWEEP CUT" in hdr
    assert re.search(r"typedef struct \{ int64_t len, best; uint64_t cut, vol, den; double conductance; \} fora_sweep_row;", code)
    m = re.search(r"typedef struct \{([^}]*)\} fora_sweep_stats;", code)
    assert m
    fields = [f.strip() for decl in m.group(1).split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    lib = ctypes.CDLL(capi.lib_path())
    for name in ("fora_hip_sweep_batch", "fora_hip_sweep_fetch", "fora_hip_sweep_clear"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert ctypes.sizeof(capi.SweepRow) == 48 and [f for f, _ in capi.SweepRow._fields_] == ["len", "best", "cut", "vol", "den", "conductance"]
    assert ctypes.sizeof(capi.SweepStats) == 64 and [f for f, _ in capi.SweepStats._fields_] == fields
    for meth in ("sweep", "sweep_fetch", "sweep_clear", "local_cluster"):
        assert callable(getattr(capi.Engine, meth))
    # NULL ctx: answered without touching the GPU
    lib.fora_hip_sweep_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int64,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.fora_hip_sweep_batch(None, None, 0, 0, 0.0, 0, None, None, None, None) == -1
    lib.fora_hip_sweep_fetch.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint64]
    assert lib.fora_hip_sweep_fetch(None, None, None, None, 0) == -1
    lib.fora_hip_sweep_clear.argtypes = [ctypes.c_void_p]
    assert lib.fora_hip_sweep_clear(None) == -1
