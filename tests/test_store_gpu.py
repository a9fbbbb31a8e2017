"""The ROW STORE on the GPU, through the C ABI (the contract of include/fora_hip.h): rows put or loaded into the store and taken
back are the rows the numpy twin (tests/store_ref.py) gives, word for word -- every comparison here is an equality -- and a
result that was taken is an ordinary held result for everything downstream."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import attention_bwd_ref as abr
import attention_ref as ar
import propagate_ref as pr
import store_ref
from conftest import pick_sources
from test_sparse_gpu import SEED, _load, _mixed_sources

pytestmark = pytest.mark.gpu
E_ARG = -1
LENS = [0, 1, 63, 64, 65, 127, 128, 129, 256, 257, 2000]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _fetch(engine, e):
    ids, vals, fix = np.zeros(e, np.int32), np.zeros(e, np.float64), np.zeros(e, np.uint64)
    engine.sparse_fetch(ids, vals, fix, cap=e)
    return ids, vals, fix


def _take(engine, rows):
    row_ptr, st = engine.store_take(rows)
    assert st["rows"] == len(rows) and st["entries"] == int(row_ptr[-1])
    return (row_ptr,) + _fetch(engine, int(row_ptr[-1]))


def _same(got, want):
    """(row_ptr, ids, vals, fix) twice: equal word for word (vals by their bits)"""
    for a, b, name in zip(got, want, ("row_ptr", "ids", "vals", "fix")):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert (a.view(np.uint64) == b.view(np.uint64)).all() if a.dtype == np.float64 else (a == b).all(), name


def _twin(store, rows):
    rp, ids, fix, vals = store_ref.take(store[0], store[1], store[2], rows)
    return rp, ids, vals, fix


def _held(engine, srcs, **kw):
    """(row_ptr, ids, vals, fix) of a query_sparse that stays held"""
    row_ptr, ids, vals, fix, _, _ = engine.query_sparse(srcs, want_fix=True, **kw)
    return row_ptr, ids, vals, fix


def _raw_take(engine, rows, nb, row_ptr_out):
    return engine._lib.fora_hip_store_take(engine._ctx, _p(rows), C.c_int(nb), _p(row_ptr_out), None)


def _raw_load(engine, row_ptr, nrows, ids, fix, append=0):
    return engine._lib.fora_hip_store_load(engine._ctx, _p(row_ptr), C.c_int64(nrows), _p(ids), _p(fix), C.c_int(append), None)


def _raw_put(engine, row_ptr, nq, append=0):
    return engine._lib.fora_hip_store_put(engine._ctx, _p(row_ptr), C.c_int(nq), C.c_int(append), None)


def test_identity(engine, tiny_dangling):
    g = tiny_dangling
    _load(engine, g, epsilon=0.5)
    srcs = _mixed_sources(g, 8100)                # a dangling source and a duplicate
    assert (g.deg[srcs] == 0).sum() == 1 and len(set(srcs.tolist())) < len(srcs)
    want = _held(engine, srcs, threshold=0.0)
    nq = len(srcs)
    st = engine.store_put(want[0])
    assert (st["rows"], st["entries"], st["store_rows"], st["store_entries"]) == (nq, int(want[0][-1]), nq, int(want[0][-1]))
    assert st["max_row"] == int(np.diff(want[0]).max())
    _same((want[0],) + _fetch(engine, int(want[0][-1])), want)      # the put left the held result alone
    info = engine.store_info()
    assert info == {"rows": nq, "entries": int(want[0][-1]), "max_row": int(np.diff(want[0]).max())}
    gen = engine.get_option("sparse_generation")
    _same(_take(engine, np.arange(nq)), want)
    assert engine.get_option("sparse_generation") > gen             # the queried result ended, the taken one is held
    assert engine.store_info() == info
    _same(_take(engine, np.arange(nq)), want)                       # the store is what it was


def test_permutation_duplicates_and_single_entry_rows(engine, tiny_dangling):
    g = tiny_dangling
    _load(engine, g, epsilon=0.5)
    live = list(pick_sources(g, 6, 8200))
    dang = list(pick_sources(g, 3, 8201, want_dangling=True))
    srcs = np.array(live[:2] + dang[:1] + live[2:] + dang[1:], dtype=np.int32)
    store = _held(engine, srcs)
    store = (store[0], store[1], store[3])
    engine.store_put(store[0])
    lens = np.diff(store[0])
    assert (lens[[2, 7, 8]] == 1).all() and lens.max() > 1
    rows = [8, 3, 3, 0, 2, 7, 7, 7, 5, 1, 2, 8, 4, 6, 0]           # every row, duplicates, rows repeated back to back, dangling rows next to each other
    _same(_take(engine, rows), _twin(store, rows))
    _same(_take(engine, [2]), _twin(store, [2]))                    # one entry in all
    _same(_take(engine, rows[::-1]), _twin(store, rows[::-1]))


def test_append_equals_one_call(engine, tiny_dangling):
    """rows put by two calls equal the rows of one call over both source lists: the batch-independence contract"""
    g = tiny_dangling
    _load(engine, g, epsilon=0.5)
    A, B = _mixed_sources(g, 8300), _mixed_sources(g, 8310)[::-1].copy()
    AB = np.concatenate([A, B])
    every = np.arange(len(AB))
    # plain rows
    engine.store_put(_held(engine, A)[0])
    st = engine.store_put(_held(engine, B)[0], append=True)
    assert st["rows"] == len(B) and st["store_rows"] == len(AB)
    got = _take(engine, every)
    _same(got, _held(engine, AB))
    # top-k rows
    k = 16
    topk = lambda s: engine.query_sparse_topk(s, k, threshold=0.0, want_fix=True)[:4]
    engine.store_put(topk(A)[0])
    engine.store_put(topk(B)[0], append=True)
    got = _take(engine, every)
    assert int(np.diff(got[0]).max()) == k
    _same(got, topk(AB))
    # seed-set rows
    la, lb = [int(s) for s in A if g.deg[s] > 0], [int(s) for s in B if g.deg[s] > 0]
    sets_a, sets_b = [la[:3], la[2:5]], [lb[:2], [lb[0]], lb[1:5]]
    seeds = lambda sets: (lambda r: (r["row_ptr"], r["ids"], r["vals"], r["fix"]))(engine.query_seeds_sparse(sets, want_fix=True))
    engine.store_put(seeds(sets_a)[0])
    engine.store_put(seeds(sets_b)[0], append=True)
    _same(_take(engine, np.arange(5)), seeds(sets_a + sets_b))
    # an append to a store that was cleared fills it
    engine.store_clear()
    engine.store_put(_held(engine, B)[0], append=True)
    _same(_take(engine, np.arange(len(B))), _held(engine, B))


def _crafted(n, seed=8400):
    """a store of rows of every length of LENS, empty rows first, last and side by side, words that include 0, 1 and 2^64 - 1"""
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = [0, 0] + LENS[1:] + [0, 0, 0, 64, 1, 0]
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([np.sort(rng.choice(n, size=L, replace=False)) for L in lens]).astype(np.int32)
    fix = rng.integers(0, 1 << 64, size=ids.size, dtype=np.uint64)
    fix[::7] = 0
    fix[1::7] = 1
    fix[2::7] = np.uint64(2**64 - 1)
    return row_ptr, ids, fix


def test_shapes_through_load(engine, tiny):
    g = tiny
    assert g.n == 2000
    _load(engine, g, epsilon=0.5)
    store = _crafted(g.n)
    R = len(store[0]) - 1
    rng = np.random.Generator(np.random.PCG64(8401))
    orders = [np.arange(R), rng.permutation(R), np.concatenate([rng.permutation(R), rng.integers(0, R, size=9)])]
    st = engine.store_load(*store)
    assert (st["rows"], st["entries"], st["max_row"], st["ids_on_device"], st["fix_on_device"]) == (R, int(store[0][-1]), 2000, 0, 0)
    assert engine.store_info() == {"rows": R, "entries": int(store[0][-1]), "max_row": 2000}
    try:
        for span in (64, 256, None):
            if span is None:
                engine.reset_options()
            else:
                engine.set_option("take_span", span)
            for rows in orders:
                _same(_take(engine, rows), _twin(store, rows))
        # the same store by two appends, loaded under a small span (the check runs over the same plan)
        engine.set_option("take_span", 64)
        cut = 9
        e = int(store[0][cut])
        engine.store_load(store[0][:cut + 1], store[1][:e], store[2][:e])
        st = engine.store_load(store[0][cut:] - e, store[1][e:], store[2][e:], append=True)
        assert st["rows"] == R - cut and st["store_rows"] == R and st["store_entries"] == int(store[0][-1])
        for rows in orders:
            _same(_take(engine, rows), _twin(store, rows))
        # the fetched doubles are the words scaled, as always
        got = _take(engine, orders[0])
        assert (got[2] == np.ldexp(got[3].astype(np.float64), -62)).all()
    finally:
        engine.reset_options()


def test_a_span_that_meets_hundreds_of_empty_rows(engine, tiny):
    """700 empty rows between two rows: the span's window is wider than what a workgroup stages in LDS (512 rows,
    fora_store.h), so take and load's check search the plan in global memory -- the same arrays"""
    g = tiny
    _load(engine, g, epsilon=0.5)
    rng = np.random.Generator(np.random.PCG64(8450))
    lens = [70] + [0] * 700 + [64, 3] + [0] * 520
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([np.sort(rng.choice(g.n, size=L, replace=False)) for L in lens if L]).astype(np.int32)
    fix = rng.integers(0, 1 << 64, size=ids.size, dtype=np.uint64)
    store = (row_ptr, ids, fix)
    R = len(lens)
    orders = [np.arange(R), np.concatenate([np.arange(R - 521, R), np.arange(0, 703)]), np.arange(R)[::-1].copy()]
    try:
        for span in (64, 256, None):
            if span is None:
                engine.reset_options()
            else:
                engine.set_option("take_span", span)
            engine.store_load(*store)                               # (the check under this span)
            for rows in orders:
                _same(_take(engine, rows), _twin(store, rows))
            bad = ids.copy()
            bad[70] = g.n                                           # the first entry behind the empty rows
            assert _raw_load(engine, row_ptr, R, bad, fix) == E_ARG
            assert "entry 70 (row 701, place 0)" in engine._lib.fora_hip_last_error(engine._ctx).decode()
            bad = ids.copy()
            bad[72] = bad[71]
            assert _raw_load(engine, row_ptr, R, bad, fix, 1) == E_ARG
            assert "entry 72 (row 701, place 2)" in engine._lib.fora_hip_last_error(engine._ctx).decode()
            _same(_take(engine, orders[0]), _twin(store, orders[0]))
    finally:
        engine.reset_options()


def test_bad_loads_leave_the_store(engine, tiny):
    g = tiny
    n = g.n
    _load(engine, g, epsilon=0.5)
    store = _crafted(n, seed=8500)
    engine.store_load(*store)
    rows = [5, 3, 12, 0, 9]
    want = _twin(store, rows)
    info = engine.store_info()
    row_ptr = np.array([0, 3, 3, 6], dtype=np.int64)
    fix = np.arange(6, dtype=np.uint64)
    ids_of = lambda *v: np.array(v, dtype=np.int32)
    bad = {
        "descending": ids_of(1, 9, 4, 0, 5, 8),
        "equal": ids_of(1, 9, 9, 0, 5, 8),
        "id == n": ids_of(1, 9, n, 0, 5, 8),
        "id == -1": ids_of(1, 9, 10, -1, 5, 8),
        "equal in the last row": ids_of(1, 9, 10, 0, 5, 5),
    }
    for append in (0, 1):
        for name, ids in bad.items():
            assert store_ref.first_bad_entry(row_ptr, ids, n) is not None
            assert _raw_load(engine, row_ptr, 3, ids, fix, append) == E_ARG, name
            msg = engine._lib.fora_hip_last_error(engine._ctx).decode()
            assert f"entry {store_ref.first_bad_entry(row_ptr, ids, n)} " in msg, (name, msg)
            assert engine.store_info() == info, name
        for name, rp in (("start", [1, 3, 3, 6]), ("decreasing", [0, 4, 3, 6]), ("negative", [0, -1, 3, 6])):
            assert _raw_load(engine, np.array(rp, dtype=np.int64), 3, bad["descending"], fix, append) == E_ARG, name
        assert _raw_load(engine, row_ptr, 3, None, fix, append) == E_ARG
        assert _raw_load(engine, row_ptr, 3, bad["equal"], None, append) == E_ARG
        assert _raw_load(engine, None, 3, bad["equal"], fix, append) == E_ARG
        assert _raw_load(engine, row_ptr, -1, bad["equal"], fix, append) == E_ARG
        assert engine.store_info() == info
        _same(_take(engine, rows), want)
    # the same ids are legal where the pair lies across a row boundary: 9 then 4, 9 then 9
    for ids in (ids_of(1, 5, 9, 4, 5, 8), ids_of(1, 5, 9, 9, 10, n - 1)):
        assert store_ref.load_ok(row_ptr, ids, n)
        engine.store_load(row_ptr, ids, fix)
        _same(_take(engine, [2, 1, 0]), _twin((row_ptr, ids, fix), [2, 1, 0]))
    # no rows, replacing: an empty store
    engine.store_load(np.zeros(1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint64))
    assert engine.store_info() == {"rows": 0, "entries": 0, "max_row": 0}


def _b64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _downstream(engine, row_ptr, n, ops):
    """propagate (f64), attention with two heads (f64, y64) and its backward pass on the held result"""
    H, Q, K, V, G = ops
    out = engine.sparse_propagate(row_ptr, H, want32=False, want64=True)[1]
    _, o64, _, y64, _ = engine.sparse_attention(row_ptr, Q, K, V, heads=2, want32=False, want64=True, want_y64=True)
    grads = engine.sparse_attention_bwd(row_ptr, Q, K, V, G, y64, heads=2, want32=False, want64=True)
    return out, o64, y64, grads[1], grads[3], grads[5]


def test_downstream_calls_on_a_taken_result(engine, small):
    g = small
    _load(engine, g, epsilon=0.5)
    pool = pick_sources(g, 10, 8600)
    k, d, dv, heads = 64, 8, 6, 2
    engine.store_put(engine.query_sparse_topk(pool, k, threshold=0.0)[0])
    rows = np.array([7, 2, 2, 9, 0, 5], dtype=np.int64)
    nq = len(rows)
    rng = np.random.Generator(np.random.PCG64(8601))
    H = pr.scaled_features(rng, g.n, 5)
    Q, K = ar.scores_operands(rng, nq, g.n, d, heads, spread=12.0)
    V = rng.standard_normal((g.n, heads * dv)).astype(np.float32)
    G = rng.standard_normal((nq, heads * dv)).astype(np.float32)
    ops = (H, Q, K, V, G)
    row_ptr, ids, vals, fix = _take(engine, rows)
    assert int(np.diff(row_ptr).max()) == k
    got = _downstream(engine, row_ptr, g.n, ops)
    # the twins on the taken arrays
    scale = float(d) ** -0.5
    w_out = pr.propagate_ref(row_ptr, ids, fix, H)[0]
    w_o64, _, w_y64, _, nan_rows = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, scale)
    assert nan_rows == 0
    w_dq, w_dk, w_dv = abr.attention_bwd_ref(row_ptr, ids, Q, K, V, G, got[2], g.n, d, dv, heads, scale)
    for a, b, name in zip(got, (w_out, w_o64, w_y64, w_dq, w_dk, w_dv), ("propagate", "attention", "y", "dq", "dk", "dv")):
        assert a.shape == b.shape and (_b64(a) == _b64(b)).all(), name
    # the same calls on a direct query of those sources
    direct = engine.query_sparse_topk(pool[rows], k, threshold=0.0, want_fix=True)[:4]
    _same((row_ptr, ids, vals, fix), direct)
    again = _downstream(engine, direct[0], g.n, ops)
    for a, b, name in zip(got, again, ("propagate", "attention", "y", "dq", "dk", "dv")):
        assert (_b64(a) == _b64(b)).all(), name


def test_lifetime_and_errors(engine, tiny_dangling):
    g = tiny_dangling
    _load(engine, g, epsilon=0.5)
    srcs = _mixed_sources(g, 8700)
    held = _held(engine, srcs)
    store = (held[0], held[1], held[3])
    engine.store_put(held[0])
    info = engine.store_info()
    rows = [3, 0, 6, 6]
    want = _twin(store, rows)
    # what leaves the store alone
    engine.sparse_clear()
    assert engine.store_info() == info
    _held(engine, srcs[:2])
    engine.sweep(srcs[:3])
    engine.set_option("take_span", 128)
    engine.set_option("tail", 0)                  # (a layout option: the workspace goes)
    engine.set_batch(3)
    try:
        engine.query(srcs[:4], want_ppr=False)
        assert engine.store_info() == info
        _same(_take(engine, rows), want)
    finally:
        engine.reset_options()
        engine.set_batch(0)
    assert engine.store_info() == info
    _same(_take(engine, rows), want)
    # a bad index ends the held result and leaves the store
    gen = engine.get_option("sparse_generation")
    out = np.zeros(3, dtype=np.int64)
    for bad in ([0, len(srcs)], [-1, 0]):
        assert _raw_take(engine, np.array(bad, dtype=np.int64), 2, out) == E_ARG
        assert engine._lib.fora_hip_sparse_fetch(engine._ctx, None, None, None, C.c_uint64(0)) == E_ARG    # nothing is held
    assert engine.get_option("sparse_generation") > gen and engine.store_info() == info
    _same(_take(engine, rows), want)
    assert _raw_take(engine, np.array([0], dtype=np.int64), 1, None) == E_ARG      # no row_ptr_out
    assert _raw_take(engine, np.array([0], dtype=np.int64), -1, out) == E_ARG
    assert _raw_take(engine, None, 1, out) == E_ARG
    assert engine._lib.fora_hip_sparse_fetch(engine._ctx, None, None, None, C.c_uint64(0)) == E_ARG
    # nb == 0 holds an empty result
    row_ptr, st = engine.store_take([])
    assert row_ptr.tolist() == [0] and st["entries"] == 0 and st["store_rows"] == info["rows"]
    assert engine._lib.fora_hip_sparse_fetch(engine._ctx, None, None, None, C.c_uint64(0)) == 0
    # a put needs the held result and its row_ptr
    assert _raw_put(engine, held[0], len(srcs)) == E_ARG                            # (the empty result is held: another row_ptr)
    engine.sparse_clear()
    assert _raw_put(engine, held[0], len(srcs)) == E_ARG
    assert _raw_put(engine, np.zeros(1, dtype=np.int64), 0) == E_ARG
    h2 = _held(engine, srcs[:3])
    wrong = h2[0].copy()
    wrong[-1] += 1
    assert _raw_put(engine, wrong, 3, 1) == E_ARG and _raw_put(engine, h2[0], 2, 1) == E_ARG and _raw_put(engine, None, 3, 1) == E_ARG
    assert engine.store_info() == info
    # put of an empty held result, appending: nothing is added
    engine.store_take([])
    st = engine.store_put(np.zeros(1, dtype=np.int64), append=True)
    assert st["rows"] == 0 and engine.store_info() == info
    # store_clear and set_graph drop the store
    for drop in (engine.store_clear, lambda: _load(engine, g, epsilon=0.5)):
        engine.store_put(_held(engine, srcs)[0])
        assert engine.store_info() == info
        drop()
        assert engine.store_info() == {"rows": 0, "entries": 0, "max_row": 0}
        assert _raw_take(engine, np.zeros(1, dtype=np.int64), 1, out) == E_ARG
        assert engine.store_take([])[0].tolist() == [0]
    # a NULL ctx is answered by every entry point
    lib, one = engine._lib, np.zeros(1, dtype=np.int64)
    assert lib.fora_hip_store_put(None, _p(one), C.c_int(0), C.c_int(0), None) == E_ARG
    assert lib.fora_hip_store_load(None, _p(one), C.c_int64(0), None, None, C.c_int(0), None) == E_ARG
    assert lib.fora_hip_store_take(None, _p(one), C.c_int(0), _p(out), None) == E_ARG
    assert lib.fora_hip_store_info(None, None, None, None) == E_ARG
    assert lib.fora_hip_store_clear(None) == E_ARG


def test_device_arrays_and_autograd():
    """store_load from torch tensors and the torch_ops functions on a taken result, in a child of their own
    (tests/store_device_child.py): torch and the library must live on one HIP runtime, so the child imports torch first."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "store_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "store device ok" in r.stdout
