"""PROPAGATE, TRANSPOSED (fora_hip_sparse_propagate_t) without a GPU: the numpy twin (tests/propagate_t_ref.py) against an
independent yardstick, the injected input's power to tell one order of a column's entries from another, the host-only tier
split and sorting network (fora_amd/csrc/fora_propt_plan.h) against brute force under the address and undefined-behaviour
sanitizers -- a stand-alone program and nothing else is sanitized -- and the library's symbols."""
import math
import os
import subprocess

import numpy as np
import pytest

import propagate_ref as pr
import propagate_t_ref as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def injected():
    rows_fix, col_lens = pt.injected_columns()
    row_ptr, ids, fix = pt.csr_of(rows_fix)
    n = rows_fix.shape[1]
    col_ptr, rows, fix_t = pt.transpose_ref(row_ptr, ids, fix, n)
    G = pr.scaled_features(np.random.Generator(np.random.PCG64(7101)), rows_fix.shape[0], 16)
    return {"n": n, "rows_fix": rows_fix, "col_lens": col_lens, "row_ptr": row_ptr, "ids": ids, "fix": fix, "col_ptr": col_ptr, "rows": rows,
            "fix_t": fix_t, "G": G}


def test_injected_input_is_what_the_gpu_test_expects(injected):
    rows_fix, col_lens, row_ptr, col_ptr = injected["rows_fix"], injected["col_lens"], injected["row_ptr"], injected["col_ptr"]
    assert rows_fix.shape == (601, 2000) and row_ptr[300] == row_ptr[301] and (np.diff(row_ptr)[np.arange(601) != 300] > 0).all()
    assert (np.diff(col_ptr) == col_lens).all()
    for L in pt.COL_LENS:
        assert (col_lens == L).sum() >= 3
    assert col_lens.max() == 600 and 10000 < col_lens.sum() < 12500
    assert int(rows_fix.max()) <= (1 << 62) // 1024
    # the transposition: column v lists (row, word) by ascending row -- restated entry by entry, without a sort
    rows, fix_t = injected["rows"], injected["fix_t"]
    for v in (int(x) for x in np.flatnonzero(col_lens >= 63)[:6]):
        lo, hi = int(col_ptr[v]), int(col_ptr[v + 1])
        want = [(i, int(rows_fix[i, v])) for i in range(rows_fix.shape[0]) if rows_fix[i, v]]
        assert [(int(r), int(w)) for r, w in zip(rows[lo:hi], fix_t[lo:hi])] == want
    assert pt.tier_counts(col_ptr) == {"short_cols": int(((col_lens >= 2) & (col_lens <= 64)).sum()), "lds_cols": int((col_lens > 64).sum()), "global_cols": 0}
    assert pt.tier_counts(col_ptr, 64)["global_cols"] == int((col_lens > 64).sum()) and pt.tier_counts(col_ptr, 64)["lds_cols"] == 0
    assert pt.tier_counts(col_ptr, 0) == {"short_cols": 0, "lds_cols": 0, "global_cols": int((col_lens >= 2).sum())}


@pytest.mark.parametrize("normalize", [False, True])
def test_twin_against_fsum(injected, normalize):
    """every output within len * 2^-52 * sum|term| of the exactly rounded sum (math.fsum) of the same terms -- the tolerance
    tests/test_propagate_cpu.py derives -- with the terms made here entry by entry from the dense rows"""
    n, rows_fix, G = injected["n"], injected["rows_fix"], injected["G"]
    out64, out32 = pt.propagate_t_ref(injected["row_ptr"], injected["ids"], injected["fix"], G, n, normalize=normalize)
    S = [sum(int(x) for x in rows_fix[i]) for i in range(rows_fix.shape[0])]
    assert max(S) < (1 << 62)                                                   # no row sum wraps
    G64 = G.astype(np.float64)
    for v in range(n):
        at = np.flatnonzero(rows_fix[:, v])
        for c in (0, 7, 15):
            terms = []
            for i in at:
                w = math.ldexp(float(int(rows_fix[i, v])), -62)
                if normalize:
                    w = w / math.ldexp(float(S[i]), -62)
                terms.append(w * float(G64[i, c]))
            exact = math.fsum(terms)
            bound = len(terms) * 2.0 ** -52 * math.fsum(abs(t) for t in terms)
            assert abs(out64[v, c] - exact) <= bound, (v, c, len(terms))
        if not at.size:
            assert (out64[v] == 0.0).all() and not np.signbit(out64[v]).any()    # a node no row keeps: +0.0
    assert (out32 == out64.astype(np.float32)).all()


def test_injected_input_tells_the_orders_apart(injected):
    """a column's sum depends on the order of its entries and on the segments: some column of three entries or more gives
    other bits with its entries reversed, and shuffled, and some column longer than 256 gives other bits without segments --
    so an implementation that skips the sort, or cuts segments elsewhere, cannot pass the bitwise GPU tests"""
    col_ptr, rows, fix_t, col_lens = injected["col_ptr"], injected["rows"], injected["fix_t"], injected["col_lens"]
    G64 = injected["G"].astype(np.float64)
    rng = np.random.Generator(np.random.PCG64(7102))
    differ = {"reversed": 0, "shuffled": 0, "unsegmented": 0}
    for v in np.flatnonzero(col_lens >= 3):
        lo, hi = int(col_ptr[v]), int(col_ptr[v + 1])
        terms = pt.column_terms(rows[lo:hi], fix_t[lo:hi], G64)
        want = pr.sum_row(terms)
        differ["reversed"] += bool((pr.sum_row(terms[::-1]) != want).any())
        differ["shuffled"] += bool((pr.sum_row(terms[rng.permutation(hi - lo)]) != want).any())
        if hi - lo > 256:
            differ["unsegmented"] += bool((pr.sum_row(terms, None) != want).any())
    print(differ, int((col_lens >= 3).sum()), int((col_lens > 256).sum()))
    assert all(x >= 1 for x in differ.values()), differ


# ---- the host-only tier split and the sorting network
@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("propt") / "propt_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "propt_plan_check.cpp")], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    return r.stdout


TIER_COLS = [
    [],
    [0], [1], [2], [0, 0, 1, 1],
    [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 0, 1],
    [5000, 2, 5000, 70, 1],
]


@pytest.mark.parametrize("option", [0, 1, 2, 64, 65, 4096, 100000, -3])
def test_tier_split_against_brute_force(plan_check, injected, option):
    for lens in TIER_COLS + [injected["col_lens"].tolist()]:
        words = _run(plan_check, "tiers", option, ",".join(map(str, lens)) or "-").split()
        assert words[-1] == "ok"
        f = {k: int(v) for k, v in (w.split("=") for w in words[:-1])}
        col_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ref = pt.tier_counts(col_ptr, option)
        assert {"short_cols": f["short"], "lds_cols": f["lds"], "global_cols": f["global"]} == ref
        assert f["columns"] == sum(1 for L in lens if L) and f["max_col"] == max(lens, default=0) and f["entries"] == sum(lens)
    assert _run(plan_check, "tiers", 0, "0,1,2,3").split()[:3] == ["short=0", "lds=0", "global=2"]
    assert _run(plan_check, "tiers", 64, "2,64,65,4097").split()[:3] == ["short=2", "lds=0", "global=2"]
    assert _run(plan_check, "tiers", 4096, "2,64,65,4096,4097").split()[:3] == ["short=2", "lds=2", "global=1"]


def test_sorting_network_sorts_runs_of_any_length(plan_check):
    assert _run(plan_check, "network").split() == ["ok"]


# ---- the symbols
def test_symbols_and_null_ctx():
    """the libraries export the two entry points and answer a NULL ctx with FORA_E_ARG without touching a GPU; the header
    declares the stats struct the binding mirrors"""
    import re
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "PROPAGATE, TRANSPOSED" in hdr
    assert capi.STRUCTS["fora_propt_stats"] is capi.PropTStats  # (its fields and size against the header: tests/test_capi_cpu.py)
    names = ("fora_hip_sparse_propagate_t", "fora_hip_sparse_transpose_fetch")
    for lib in (capi.load(), capi.load(capi.TEST_LIB)):
        for name in names:
            assert hasattr(lib, name) and name in capi.SYMBOLS and re.search(r"\bint\s+" + name + r"\s*\(", code), name
        fn = lib.fora_hip_sparse_propagate_t
        rp = np.zeros(2, dtype=np.int64)
        out = np.full(4, 7.0, dtype=np.float32)
        assert fn(None, rp.ctypes.data, 1, None, 0, 4, 4, 0, out.ctypes.data, None, 4, None) == -1
        assert (out == 7.0).all()
        fetch = lib.fora_hip_sparse_transpose_fetch
        assert fetch(None, rp.ctypes.data, 1, None, None, None, None, 0) == -1
    for meth in ("sparse_propagate_t", "sparse_transpose_fetch"):
        assert callable(getattr(capi.Engine, meth))
    # the package stays free of torch; the autograd function is a module of its own
    init = open(os.path.join(ROOT, "fora_amd", "__init__.py")).read()
    assert "torch_ops" not in init and os.path.exists(os.path.join(ROOT, "fora_amd", "torch_ops.py"))
