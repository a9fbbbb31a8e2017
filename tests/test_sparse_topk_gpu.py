"""Top-k sparse rows (fora_hip_query_sparse_topk_batch, the SPARSE RESULTS, TOP-K contract) on the GPU.

The yardstick never passes through the new code: the dense rows of the same context (Engine.query_fix, pinned to
oracle/fora_twin.c by the parity tests) or the injected rows themselves, through the numpy twin tests/sparse_topk_ref.py.
Every comparison is an equality, and every test asserts through the top-k stats that it reached the path it is about."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import propagate_ref as pr
import propagate_t_ref as pt
from conftest import pick_sources
from growth_case import growth_case, growths_with_entries_to_keep
from sparse_topk_ref import check_topk, topk_csr
from test_sparse_gpu import SEED, _load, _mixed_sources, _raw_fetch, thr_fix_of

pytestmark = pytest.mark.gpu
FIX_ONE = 1 << 62
LDS_MAX = 18432
KS = (1, 2, 7, 64, 10 ** 9)


@pytest.mark.parametrize("gname", ["tiny_dangling", "small"])
def test_query_rows_equal_the_twin(engine, request, gname):
    g = request.getfixturevalue(gname)
    srcs = _mixed_sources(g, 4100)
    live = g.deg[srcs] > 0
    assert int((~live).sum()) == (1 if gname == "tiny_dangling" else 0)
    _load(engine, g, epsilon=0.5)
    try:
        for with_idx in (False, True):
            if with_idx:
                engine.build_index()
            want, _, wst = engine.query_fix(srcs, with_idx=with_idx)
            for t in (0.0, 1.0 / g.n):
                thr = thr_fix_of(t)
                plain = engine.query_sparse(srcs, with_idx=with_idx, threshold=t, want_fix=True)
                cut_seen = 0
                for k in KS:
                    row_ptr, ids, vals, fix, st, sp, tk = engine.query_sparse_topk(srcs, k, with_idx=with_idx, threshold=t, want_fix=True)
                    lens = check_topk(want, thr, k, row_ptr, ids, fix, sp, tk, live=live)
                    assert (vals == np.ldexp(fix.astype(np.float64), -62)).all()
                    for name in st.dtype.names:
                        assert (st[name] == wst[name]).all(), name
                    assert tk["chunks"] >= 1 and tk["select_ms"] >= 0 and sp["compact_ms"] >= 0 and sp["batches"] == 1
                    cut_seen += tk["cut_rows"]
                    for i, s in enumerate(srcs):
                        if not live[i]:
                            assert row_ptr[i + 1] - row_ptr[i] == 1 and ids[row_ptr[i]] == s and fix[row_ptr[i]] == FIX_ONE
                    if k == 10 ** 9:   # nothing cut: the plain call's arrays, word for word
                        assert tk["cut_rows"] == 0 and k >= lens.max()
                        assert (row_ptr == plain[0]).all() and (ids == plain[1]).all() and (vals == plain[2]).all() and (fix == plain[3]).all()
                assert cut_seen > 0
    finally:
        engine.clear_index()


def _ring(oracle, n):
    v = np.arange(n, dtype=np.int32)
    return oracle.Graph.from_edges(n, n, v, (v + 1) % n)


def _three_class_row(n, big_at, equal_at, E=5000):
    """distinct words below E everywhere, the word E at equal_at, distinct words above E at big_at"""
    w = 1 + np.arange(n, dtype=np.uint64) % np.uint64(E - 1)
    w[np.asarray(equal_at, dtype=np.int64)] = E
    w[np.asarray(big_at, dtype=np.int64)] = np.uint64(E + 1) + np.arange(len(big_at), dtype=np.uint64) * np.uint64(1 << 40)
    return w


def _injected_cases(n):
    """(name, k, rows [nq, n]) -- every dense row is its own candidate list, position = id"""
    rng = np.random.Generator(np.random.PCG64(9100 + n))
    cases = []
    equal = np.full((3, n), 7, dtype=np.uint64)          # three rows: with an odd n the middle one starts at an odd word
    for k in (1, 63, 64, 65, n - 1, n):
        cases.append(("all equal", k, equal))
    # k - 1 distinct large words and a run of equal ones, the equal entries taken across a wave (63 | 64, 255 | 256), a
    # workgroup step (1023 | 1024) and at the end of the row
    big = [10, 500, 1500]
    rows = [_three_class_row(n, big, [p - 1, p, p + 1]) for p in (64, 256, 1024)] + [_three_class_row(n, big, [n - 3, n - 2, n - 1])]
    cases.append(("equal across a boundary, two of three", len(big) + 2, np.stack(rows)))
    cases.append(("equal across a boundary, all three", len(big) + 3, np.stack(rows)))
    cases.append(("equal across a boundary, one of three", len(big) + 1, np.stack(rows)))
    long_run = np.full(n, 5000, dtype=np.uint64)
    long_run[[0, 3, 64, 700, 1024, 1998, n - 1]] = np.uint64(1 << 50) + np.arange(7, dtype=np.uint64)
    cases.append(("k - 1 large words and a long run of equal ones", 8, np.stack([long_run, long_run[::-1].copy()])))
    cases.append(("... two of the run", 9, np.stack([long_run, long_run[::-1].copy()])))
    # words that differ in one byte only: every pass but one sees a single bin
    perm = rng.permutation(n).astype(np.uint64) % np.uint64(256)
    cases.append(("one byte differs", 100, np.stack([np.uint64(0x0101010101010101) ^ (perm << np.uint64(8 * b)) for b in range(8)])))
    # 2^62 (the top byte is 0x40) and words above it, as a seed set can give
    r = rng.integers(1, 1 << 61, size=n, dtype=np.uint64)
    r2 = r.copy()
    r[n // 2] = FIX_ONE
    r2[[5, n - 1]] = np.uint64(FIX_ONE) + np.array([9, 9], dtype=np.uint64)
    r2[77] = FIX_ONE
    for k in (1, 3):
        cases.append(("a row containing 2^62", k, np.stack([r, r2])))
    # rows of len 0, 1, k - 1, k and k + 1 (k = 5), zeros between the entries
    short = np.zeros((5, n), dtype=np.uint64)
    for i, L in enumerate((0, 1, 4, 5, 6)):
        short[i, rng.choice(n, L, replace=False)] = rng.integers(1, 1 << 40, size=L, dtype=np.uint64)
    cases.append(("rows of len 0, 1, k - 1, k, k + 1", 5, short))
    cases.append(("short and long rows, lds_cap 64 between them", 5, np.concatenate([short, rows[0][None, :]])))
    return cases


@pytest.mark.parametrize("n", [2000, 2001])
def test_injected_rows(engine_test, oracle, tiny, n):
    """even n: the tiny preset; odd n: a ring (slabs and rows start on odd words) -- the rows are injected, the graph only
    gives n.  Every case under both tiers, one and many chunks, and batches of two rows: identical bits, the twin's."""
    e = engine_test
    g = tiny if n == 2000 else _ring(oracle, n)
    assert g.n == n
    _load(e, g, epsilon=0.5)
    cases = _injected_cases(n)
    twins = [topk_csr(rows, 1, k) for _, k, rows in cases]
    try:
        for batch in (0, 2):
            e.set_batch(batch)
            for lds in (LDS_MAX, 0, 64):
                e.set_option("topk_lds_cap", lds)
                for cand in (0, 1, 2 * n):
                    e.set_option("topk_cand", cand)
                    for (name, k, rows), (want_ptr, want_ids, want_fix, lens) in zip(cases, twins):
                        where = (name, k, batch, lds, cand)
                        row_ptr, sp, tk = e.test_sparse_topk_rows(rows, k)
                        assert (row_ptr == want_ptr).all(), where
                        ids, fix = np.zeros(sp["entries"], np.int32), np.zeros(sp["entries"], np.uint64)
                        assert _raw_fetch(e, ids, None, fix, sp["entries"]) == 0
                        assert (ids == want_ids).all() and (fix == want_fix).all(), where
                        cut = lens > k
                        assert tk["cut_rows"] == int(cut.sum()) and tk["support"] == int(lens.sum()) and tk["k"] == k, where
                        assert tk["lds_rows"] == int((cut & (lens <= lds)).sum()) and tk["global_rows"] == int((cut & (lens > lds)).sum()), where
                        assert sp["entries"] == int(want_ptr[-1]) and sp["max_row"] == int(np.diff(want_ptr).max()), where
                        nbatch = 1 if batch == 0 else -(-len(rows) // 2)
                        assert sp["batches"] == nbatch, where
                        filled = int((lens > 0).sum())
                        if cand == 1 and batch == 0 and filled > 1:
                            assert tk["chunks"] > 1, where            # a chunk per row (empty rows ride along)
                        if cand == 0:
                            assert tk["chunks"] == nbatch, where
        # the tiers were all reached over the cases
        assert any((l > k).any() for (_, k, _), (_, _, _, l) in zip(cases, twins))
    finally:
        e.reset_options()
        e.set_batch(0)


def test_growth_with_entries_to_keep(engine, small):
    """the held arrays grow across batches with written entries to carry over, every live row cut"""
    g, srcs = growth_case(engine, small)
    engine.set_batch(1)
    try:
        want, _, wst = engine.query_fix(srcs)
        lens = (want != 0).sum(axis=1)
        k = int(lens[1:].min()) - 1
        held = np.minimum(lens, k)
        print("row lengths", lens.tolist(), "k", k, "growths with entries to keep", growths_with_entries_to_keep(held))
        assert lens[0] == 2 and growths_with_entries_to_keep(held) >= 2
        engine.sparse_clear()
        row_ptr, ids, vals, fix, st, sp, tk = engine.query_sparse_topk(srcs, k, threshold=0.0, want_fix=True)
        check_topk(want, 1, k, row_ptr, ids, fix, sp, tk)
        assert sp["batches"] == 6 and tk["cut_rows"] == 5 and tk["chunks"] == 6
    finally:
        engine.set_batch(0)


def _held(engine, g, k=7):
    srcs = _mixed_sources(g, 4100)
    row_ptr, ids, vals, fix, st, sp, tk = engine.query_sparse_topk(srcs, k, threshold=0.0, want_fix=True)
    assert tk["cut_rows"] == int((g.deg[srcs] > 0).sum()) > 0 and sp["max_row"] == k
    return srcs, row_ptr, ids, fix


def test_downstream_of_a_held_topk_result(engine, tiny_dangling):
    """sparse_propagate, sparse_propagate_t, sparse_transpose_fetch and Engine.propagate(topk=) on top-k rows: the twins of
    the two products fed the top-k CSR, bit for bit"""
    g = tiny_dangling
    _load(engine, g, epsilon=0.5)
    srcs, row_ptr, ids, fix = _held(engine, g)
    nq = len(srcs)
    rng = np.random.Generator(np.random.PCG64(9200))
    d = 19
    H, G = pr.scaled_features(rng, g.n, d), pr.scaled_features(rng, nq, d)
    for bf16 in (False, True):
        Hx, Gx = (pr.to_bf16_bits(H), pr.to_bf16_bits(G)) if bf16 else (H, G)
        for normalize in (False, True):
            want64, want32 = pr.propagate_ref(row_ptr, ids, fix, Hx, normalize=normalize, bf16=bf16)
            o32, o64, ps = engine.sparse_propagate(row_ptr, Hx, normalize=normalize, bf16=bf16, want64=True)
            assert (o64.view(np.uint64) == want64.view(np.uint64)).all() and (o32.view(np.uint32) == want32.view(np.uint32)).all()
            assert ps["entries"] == int(row_ptr[-1]) and ps["max_row"] == 7
            t64, t32 = pt.propagate_t_ref(row_ptr, ids, fix, Gx, g.n, normalize=normalize, bf16=bf16)
            b32, b64, _ = engine.sparse_propagate_t(row_ptr, Gx, normalize=normalize, bf16=bf16, want64=True)
            assert (b64.view(np.uint64) == t64.view(np.uint64)).all() and (b32.view(np.uint32) == t32.view(np.uint32)).all()
    col_ptr, rows, fix_t = pt.transpose_ref(row_ptr, ids, fix, g.n)
    c, r, v, f = engine.sparse_transpose_fetch(row_ptr, want_fix=True)
    assert (c == col_ptr).all() and (r == rows).all() and (f == fix_t).all() and (v == pr.weights(fix_t)).all()
    # Engine.propagate(topk=k): the same product in one call, chunked or not; topk=None stays the full rows
    want64, want32 = pr.propagate_ref(row_ptr, ids, fix, H, normalize=True)
    for chunk in (None, 3):
        out = engine.propagate(srcs, H, threshold=0.0, normalize=True, want64=True, chunk=chunk, topk=7)
        assert (out["out64"].view(np.uint64) == want64.view(np.uint64)).all() and (out["out32"].view(np.uint32) == want32.view(np.uint32)).all()
    full = engine.query_sparse(srcs, threshold=0.0, want_fix=True)
    f64, _ = pr.propagate_ref(full[0], full[1], full[3], H, normalize=True)
    out = engine.propagate(srcs, H, threshold=0.0, normalize=True, want64=True)
    assert (out["out64"].view(np.uint64) == f64.view(np.uint64)).all() and not (f64 == want64).all()


def _fetch_ok(engine, cap):
    buf = np.zeros(max(cap, 1), np.int32)
    return _raw_fetch(engine, buf, None, None, buf.size)


def test_lifetime_and_errors(engine, small):
    import fora_amd
    g = small
    _load(engine, g, epsilon=0.5)
    ok = pick_sources(g, 2, 4600)
    lib, ctx = engine._lib, engine._ctx
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(k, t=0.0, row_ptr=True, nq=2, c=ctx):
        rp = np.zeros(3, np.int64)
        return lib.fora_hip_query_sparse_topk_batch(c, p(ok), C.c_int(nq), C.c_int(0), C.c_double(t), C.c_int64(k),
                                                    p(rp) if row_ptr else None, None, None, None)

    # a bad k and a bad threshold behave alike: FORA_E_ARG, and the result held before the call is gone (the call ends the
    # held result before it looks at either), "sparse_generation" having moved once
    for bad in (dict(k=0), dict(k=-1), dict(k=-(1 << 63)), dict(k=5, t=float("nan")), dict(k=5, t=1.5), dict(k=5, row_ptr=False)):
        assert call(5) == 0 and _fetch_ok(engine, 10) == 0
        gen = engine.get_option("sparse_generation")
        assert call(**bad) == -1, bad
        assert _fetch_ok(engine, 10) == -1, bad
        assert engine.get_option("sparse_generation") == gen + 1, bad
        assert call(**bad) == -1 and engine.get_option("sparse_generation") == gen + 1   # nothing held: nothing more to end
    # ... exactly as the plain call treats its bad threshold
    assert call(5) == 0
    gen = engine.get_option("sparse_generation")
    with pytest.raises(fora_amd.ForaError):
        engine.query_sparse(ok, threshold=float("nan"))
    assert _fetch_ok(engine, 10) == -1 and engine.get_option("sparse_generation") == gen + 1
    with pytest.raises(fora_amd.ForaError) as ei:
        engine.query_sparse_topk(ok, 0)
    assert ei.value.code == -1
    assert call(5, c=None) == -1                            # NULL ctx: answered without touching the GPU
    assert call(5, nq=-1) == -1
    # nq = 0 holds an empty result
    row_ptr, ids, vals, st, sp, tk = engine.query_sparse_topk(np.zeros(0, np.int32), 3)
    assert (row_ptr == [0]).all() and ids.size == 0 and sp["entries"] == 0 and tk["cut_rows"] == 0
    assert _fetch_ok(engine, 0) == 0
    # a held sweep profile is intact after a top-k call; the generation moves; sparse_clear drops the result
    prof = engine.sweep(ok, want_profile=True)
    engine.sparse_clear()                                   # (the empty result: from nothing held, one step to held)
    gen = engine.get_option("sparse_generation")
    row_ptr, ids, vals, fix, st, sp, tk = engine.query_sparse_topk(ok, 5, want_fix=True)
    assert engine.get_option("sparse_generation") == gen + 1 and sp["entries"] == 10 and tk["cut_rows"] == 2
    again = engine.sweep_fetch(int(prof["row_ptr"][-1]))
    assert all((a == b).all() for a, b in zip(again, (prof["ids"], prof["cut"], prof["vol"])))
    want, _, _ = engine.query_fix(ok)
    check_topk(want, thr_fix_of(1.0 / g.n), 5, row_ptr, ids, fix, sp, tk)
    i2, f2 = np.zeros(10, np.int32), np.zeros(10, np.uint64)
    assert _raw_fetch(engine, i2, None, f2, 10) == 0 and (i2 == ids).all() and (f2 == fix).all()   # any number of times
    engine.sparse_clear()
    assert _fetch_ok(engine, 10) == -1 and engine.get_option("sparse_generation") == gen + 2
    # the two options are options like the others: set, read, undone by "reset"
    engine.set_option("topk_lds_cap", 64)
    engine.set_option("topk_cand", 1000)
    assert engine.get_option("topk_lds_cap") == 64 and engine.get_option("topk_cand") == 1000
    engine.reset_options()
    assert engine.get_option("topk_lds_cap") == LDS_MAX and engine.get_option("topk_cand") == 0


def test_device_fetch_and_autograd():
    """query_sparse_topk(device=True) and one forward and backward pass of ppr_propagate over top-k rows, in a child of
    their own (tests/sparse_topk_device_child.py): torch must be imported before the library is loaded."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "sparse_topk_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "sparse topk device ok" in r.stdout
