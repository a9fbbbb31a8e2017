"""COLUMNS on the GPU, through the C ABI (the contract of include/fora_hip.h): fora_hip_sparse_compact re-expresses the held sparse
result over its own columns.  The columns and the local ids are the numpy twin's (tests/cols_ref.py), and every call on the
compacted result with the operand rows X[cols] gives the bits of the same call on the uncompacted result with X -- every
comparison here is an equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import attention_ref as ar
import cols_ref
from conftest import pick_sources
from test_sparse_gpu import _load, _mixed_sources

pytestmark = pytest.mark.gpu
E_ARG = -1
SPECIAL = [0, 1, 62, 63, 64, 65, 127, 128, 1998, 1999]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _fetch(engine, e):
    ids, vals, fix = np.zeros(e, np.int32), np.zeros(e, np.float64), np.zeros(e, np.uint64)
    engine.sparse_fetch(ids, vals, fix, cap=e)
    return ids, vals, fix


def _raw_compact(engine, row_ptr, nq, out):
    return engine._lib.fora_hip_sparse_compact(engine._ctx, _p(row_ptr), C.c_int(nq), _p(out), None)


def _raw_cols_fetch(engine, cols, cap):
    return engine._lib.fora_hip_sparse_cols_fetch(engine._ctx, _p(cols), C.c_uint64(cap))


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.itemsize]) if x.dtype.kind == "f" else x


def _eq(a, b, name):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, name
    assert (_bits(a) == _bits(b)).all(), name


def _check_twin(engine, n, held):
    """compact the held result (row_ptr, ids, vals, fix) and hold everything to the twin; returns cols"""
    row_ptr, ids, vals, fix = held
    e = int(row_ptr[-1])
    kept = row_ptr.copy()
    gen = engine.get_option("sparse_generation")
    assert engine.get_option("sparse_cols") == n == engine.held_cols
    cols, st = engine.sparse_compact(row_ptr)
    want_cols, want_local = cols_ref.compact(ids)
    got = _fetch(engine, e)
    _eq(cols, want_cols, "cols")
    _eq(got[0], want_local, "local ids")
    _eq(got[1], vals, "vals")
    _eq(got[2], fix, "fix")
    _eq(row_ptr, kept, "row_ptr")
    nc = int(want_cols.size)
    assert (st["entries"], st["cols"], st["words"]) == (e, nc, -(-n // 64) if e else 0) and st["cols_ms"] >= 0
    assert engine.get_option("sparse_cols") == nc == engine.held_cols
    assert engine.get_option("sparse_generation") > gen
    assert (cols[got[0]] == ids).all()
    return cols


def test_twin_on_plain_topk_and_seed_set_results(engine, tiny_dangling):
    g = tiny_dangling
    _load(engine, g, epsilon=0.5)
    srcs = _mixed_sources(g, 9100)                # a dangling source and a duplicate
    assert (g.deg[srcs] == 0).sum() == 1 and len(set(srcs.tolist())) < len(srcs)
    cols = _check_twin(engine, g.n, engine.query_sparse(srcs, want_fix=True)[:4])
    assert 1 < cols.size < g.n
    cols = _check_twin(engine, g.n, engine.query_sparse_topk(srcs, 16, threshold=0.0, want_fix=True)[:4])
    assert 16 <= cols.size <= 16 * len(srcs)
    live = [int(s) for s in srcs if g.deg[s] > 0]
    r = engine.query_seeds_sparse([live[:3], live[2:5], [live[0]]], want_fix=True)
    _check_twin(engine, g.n, (r["row_ptr"], r["ids"], r["vals"], r["fix"]))


def _crafted(n, lens, seed, singles=0):
    """rows of these lengths whose ids are the ids of SPECIAL that fit, then filler; `singles` more rows that hold the one id 63"""
    rng = np.random.Generator(np.random.PCG64(seed))
    special = [v for v in SPECIAL if v < n]
    rows = []
    for L in lens:
        if L >= n:
            rows.append(np.arange(n))
            continue
        first = special[:L] if L >= len(special) else list(rng.choice(special, size=L, replace=False))
        rest = rng.choice(np.setdiff1d(np.arange(n), special), size=L - len(first), replace=False)
        rows.append(np.sort(np.concatenate([first, rest]).astype(np.int64)))
    rows += [np.array([63])] * singles
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ids = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    fix = rng.integers(1, 1 << 50, size=ids.size, dtype=np.uint64)
    return row_ptr, ids, fix


def _take_compact_check(engine, n, store, rows):
    row_ptr, _ = engine.store_take(rows)
    e = int(row_ptr[-1])
    return _check_twin(engine, n, (row_ptr,) + _fetch(engine, e))


def test_crafted_ids_through_store_load(engine, tiny):
    g = tiny
    assert g.n == 2000
    _load(engine, g, epsilon=0.5)
    lens = [0, 1, 63, 64, 65, 257, 2000]
    store = _crafted(g.n, lens, 9200, singles=300)
    R = len(store[0]) - 1
    assert R == len(lens) + 300
    engine.store_load(*store)
    every = np.arange(R)
    try:
        for block in (1, 4, None):
            if block is None:
                engine.reset_options()
            else:
                engine.set_option("cols_block", block)
            cols = _take_compact_check(engine, g.n, store, every)        # a row holds every id: nc == n, the identity
            assert cols.size == g.n
            cols = _take_compact_check(engine, g.n, store, every[:6])    # without it
            assert set(SPECIAL) <= set(cols.tolist()) and cols.size < g.n
            cols = _take_compact_check(engine, g.n, store, every[7:])    # 300 rows of the same single id
            assert cols.tolist() == [63]
            cols = _take_compact_check(engine, g.n, store, [1, 0, 7, 1])
            assert cols.size <= 2
    finally:
        engine.reset_options()


def test_more_block_totals_than_the_scan_has_threads(engine, small):
    """n = 32 000 is 500 bitmap words; with cols_block = 1 that is 500 block totals, so the one workgroup of k_cols_scan loops"""
    g = small
    assert g.n == 32000
    _load(engine, g, epsilon=0.5)
    store = _crafted(g.n, [0, 1, 64, 700, 65, 3000, 257], 9300, singles=3)
    engine.store_load(*store)
    R = len(store[0]) - 1
    try:
        for block in (1, 4, None):
            if block is None:
                engine.reset_options()
            else:
                engine.set_option("cols_block", block)
            cols = _take_compact_check(engine, g.n, store, np.arange(R)[::-1].copy())
            assert 3000 < cols.size < 5000 and cols[-1] > 31000
    finally:
        engine.reset_options()


def _bf16(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _shared_rows(n, lens, seed, pool=900):
    """rows of these lengths over a pool of `pool` nodes: the rows share most of their ids, as PPR rows share hubs"""
    rng = np.random.Generator(np.random.PCG64(seed))
    nodes = np.sort(rng.choice(n, size=pool, replace=False))
    rows = [np.sort(rng.choice(nodes, size=L, replace=False)) for L in lens]
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate(rows).astype(np.int32)
    fix = rng.integers(1, 1 << 50, size=ids.size, dtype=np.uint64)
    return row_ptr, ids, fix


@pytest.fixture(scope="module")
def operands():
    """the operands over all n = 32 000 nodes, made once"""
    n, nq, heads, d, dv = 32000, 7, 2, 8, 6
    rng = np.random.Generator(np.random.PCG64(9400))
    H64 = rng.standard_normal((n, 64)).astype(np.float32)
    G64 = rng.standard_normal((nq, 64)).astype(np.float32)
    Q, K = ar.scores_operands(rng, nq, n, d, heads, spread=6.0)
    V = rng.standard_normal((n, heads * dv)).astype(np.float32)
    G = rng.standard_normal((nq, heads * dv)).astype(np.float32)
    return {"n": n, "nq": nq, "heads": heads, "d": d, "dv": dv, "H64": H64, "G64": G64, "Q": Q, "K": K, "V": V, "G": G}


def _all_calls(engine, row_ptr, ops, sel):
    """every call on the held rows; sel: the rows of the column-sided operands to pass (slice(None): all n).  Returns
    (row-sided outputs, column-sided outputs, the transposition), each a dict"""
    e = int(row_ptr[-1])
    rows, cols, heads = {}, {}, ops["heads"]
    values = np.random.Generator(np.random.PCG64(9401)).standard_normal(e)
    for d in (1, 64):
        H, Gd = np.ascontiguousarray(ops["H64"][sel, :d]), np.ascontiguousarray(ops["G64"][:, :d])
        for name, feat, bf in (("f32", H, False), ("bf16", _bf16(H), True)):
            for norm in (False, True):
                o32, o64, _ = engine.sparse_propagate(row_ptr, feat, normalize=norm, want32=True, want64=True, bf16=bf)
                rows[f"prop {name} d{d} norm{norm} 32"], rows[f"prop {name} d{d} norm{norm} 64"] = o32, o64
            o32, o64, _ = engine.sparse_propagate(row_ptr, feat, want32=True, want64=True, bf16=bf, values=values)
            rows[f"prop {name} d{d} values 32"], rows[f"prop {name} d{d} values 64"] = o32, o64
            o32, o64, _ = engine.sparse_sddmm(row_ptr, Gd, feat, want32=True, want64=True, b_bf16=bf)
            rows[f"sddmm {name} d{d} 32"], rows[f"sddmm {name} d{d} 64"] = o32, o64
        for norm in (False, True):
            o32, o64, _ = engine.sparse_propagate_t(row_ptr, Gd, normalize=norm, want32=True, want64=True)
            cols[f"prop_t d{d} norm{norm} 32"], cols[f"prop_t d{d} norm{norm} 64"] = o32, o64
        o32, o64, _ = engine.sparse_propagate_t(row_ptr, Gd, want32=True, want64=True, values=values)
        cols[f"prop_t d{d} values 32"], cols[f"prop_t d{d} values 64"] = o32, o64
    d, dv = ops["d"], ops["dv"]
    K, V = np.ascontiguousarray(ops["K"][sel]), np.ascontiguousarray(ops["V"][sel])
    for h in (1, 2):
        Qh, Kh, Vh, Gh = ops["Q"][:, :h * d], K[:, :h * d], V[:, :h * dv], ops["G"][:, :h * dv]
        Qh, Kh, Vh, Gh = (np.ascontiguousarray(x) for x in (Qh, Kh, Vh, Gh))
        o32, o64, _, y64, st = engine.sparse_attention(row_ptr, Qh, Kh, Vh, heads=h, want32=True, want64=True, want_y64=True)
        rows[f"attn h{h} 32"], rows[f"attn h{h} 64"], rows[f"attn h{h} y"] = o32, o64, y64
        rows[f"attn h{h} split"] = np.array([st["short_rows"], st["long_rows"], st["nan_rows"]])
        dq32, dq64, dk32, dk64, dv32, dv64, _ = engine.sparse_attention_bwd(row_ptr, Qh, Kh, Vh, Gh, y64, heads=h, want32=True, want64=True)
        rows[f"dq h{h} 32"], rows[f"dq h{h} 64"] = dq32, dq64
        cols[f"dk h{h} 32"], cols[f"dk h{h} 64"], cols[f"dv h{h} 32"], cols[f"dv h{h} 64"] = dk32, dk64, dv32, dv64
    col_ptr, trows, tvals, tfix = engine.sparse_transpose_fetch(row_ptr, want_fix=True)
    return rows, cols, {"col_ptr": col_ptr, "rows": trows, "vals": tvals, "fix": tfix}


@pytest.mark.parametrize("attn_short", [None, 48])
def test_same_bits_as_the_full_column_space(engine, small, operands, attn_short):
    """rows of 5 .. 300 entries: with attn_short = 48 rows and columns lie on both sides of it, by default (256) the row of 300
    alone is a longer one"""
    g, ops = small, operands
    n, nq = g.n, ops["nq"]
    assert n == ops["n"]
    _load(engine, g, epsilon=0.5)
    store = _shared_rows(n, [5, 40, 64, 0, 130, 300, 48], 9402)
    assert len(store[0]) - 1 == nq
    engine.store_load(*store)
    try:
        if attn_short is not None:
            engine.set_option("attn_short", attn_short)
        row_ptr, _ = engine.store_take(np.arange(nq))
        full_rows, full_cols, full_t = _all_calls(engine, row_ptr, ops, slice(None))
        cols, _ = engine.sparse_compact(row_ptr)
        nc = cols.size
        assert nc == np.unique(store[1]).size and nc < n // 30
        loc_rows, loc_cols, loc_t = _all_calls(engine, row_ptr, ops, cols)
    finally:
        engine.reset_options()
    for h in (1, 2):
        short, lng, nan = full_rows[f"attn h{h} split"]
        assert nan == 0 and lng >= 1 and short >= 1 and (attn_short is None or lng >= 3)
    assert full_rows.keys() == loc_rows.keys() and full_cols.keys() == loc_cols.keys()
    for name in full_rows:
        _eq(loc_rows[name], full_rows[name], name)
    outside = np.setdiff1d(np.arange(n), cols)
    for name in full_cols:
        assert full_cols[name].shape[0] == n and loc_cols[name].shape[0] == nc, name
        _eq(loc_cols[name], full_cols[name][cols], name)
        assert (_bits(full_cols[name][outside]) == 0).all(), name
        assert np.abs(loc_cols[name]).sum() > 0, name
    # the transposition: nc + 1 entries of col_ptr, every column non-empty, the same lists
    counts = np.diff(full_t["col_ptr"])
    assert full_t["col_ptr"].shape == (n + 1,) and loc_t["col_ptr"].shape == (nc + 1,)
    assert (counts[outside] == 0).all() and (counts[cols] > 0).all()
    _eq(loc_t["col_ptr"], np.concatenate([[0], np.cumsum(counts[cols])]).astype(np.int64), "col_ptr")
    for name in ("rows", "vals", "fix"):
        _eq(loc_t[name], full_t[name], "transposed " + name)


def test_lifetime_and_errors(engine, tiny_dangling):
    g = tiny_dangling
    n = g.n
    _load(engine, g, epsilon=0.5)
    lib = engine._lib
    one = np.zeros(2, dtype=np.int64)
    # nothing held
    engine.sparse_clear()
    assert _raw_compact(engine, np.zeros(1, dtype=np.int64), 0, one) == E_ARG
    assert _raw_cols_fetch(engine, np.zeros(4, np.int32), 4) == E_ARG
    srcs = _mixed_sources(g, 9500)
    H = np.random.Generator(np.random.PCG64(9501)).standard_normal((n, 3)).astype(np.float32)
    sets = [[int(s) for s in srcs if g.deg[s] > 0][:3], [int(srcs[0])]]
    want_p = engine.propagate(srcs, H, want64=True, chunk=3)["out64"]          # (with nothing compacted: what they must give below)
    want_ps = engine.propagate_seeds(sets, None, H, want64=True)["out64"]
    row_ptr, ids, vals, fix = engine.query_sparse_topk(srcs, 32, threshold=0.0, want_fix=True)[:4]
    nq, e = len(srcs), int(row_ptr[-1])
    engine.store_put(row_ptr)
    info = engine.store_info()
    before = engine.sparse_propagate(row_ptr, H, want64=True)[1]
    # bad arguments change nothing
    gen = engine.get_option("sparse_generation")
    assert _raw_cols_fetch(engine, np.zeros(n, np.int32), n) == E_ARG                 # not compacted yet
    assert _raw_compact(engine, row_ptr, nq, None) == E_ARG                           # NULL ncols_out
    wrong = row_ptr.copy()
    wrong[-1] += 1
    assert _raw_compact(engine, wrong, nq, one) == E_ARG and _raw_compact(engine, row_ptr, nq - 1, one) == E_ARG
    assert _raw_compact(engine, None, nq, one) == E_ARG
    assert engine.get_option("sparse_generation") == gen and engine.get_option("sparse_cols") == n
    _eq(_fetch(engine, e)[0], ids, "ids")
    # the compaction, then a second one
    cols, _ = engine.sparse_compact(row_ptr)
    nc = cols.size
    assert 0 < nc < n
    gen = engine.get_option("sparse_generation")
    local = _fetch(engine, e)[0]
    assert _raw_compact(engine, row_ptr, nq, one) == E_ARG
    assert "compacted already" in lib.fora_hip_last_error(engine._ctx).decode()
    assert engine.get_option("sparse_generation") == gen and engine.get_option("sparse_cols") == nc
    _eq(_fetch(engine, e)[0], local, "local ids")
    # cols_fetch: a short cap; the exact one
    assert _raw_cols_fetch(engine, np.zeros(nc, np.int32), nc - 1) == E_ARG
    again = np.zeros(nc, np.int32)
    assert _raw_cols_fetch(engine, again, nc) == 0
    _eq(again, cols, "cols")
    # the store holds node ids: a put of the compacted result is refused, the store is what it was
    from fora_amd import capi
    st = capi.StoreStats()
    assert lib.fora_hip_store_put(engine._ctx, _p(row_ptr), C.c_int(nq), C.c_int(0), C.byref(st)) == E_ARG
    assert lib.fora_hip_store_put(engine._ctx, _p(row_ptr), C.c_int(nq), C.c_int(1), None) == E_ARG
    assert engine.store_info() == info
    # a feat over all n nodes is refused by the binding; the local one gives the bits of before
    with pytest.raises(ValueError):
        engine.sparse_propagate(row_ptr, H, want64=True)
    _eq(engine.sparse_propagate(row_ptr, H[cols], want64=True)[1], before, "propagate")
    # propagate and propagate_seeds replace the held result: over a compacted one they still take a feat over all n nodes (and
    # no other), and give the bits they give otherwise
    for call, want in ((lambda X: engine.propagate(srcs, X, want64=True, chunk=3), want_p),
                       (lambda X: engine.propagate_seeds(sets, None, X, want64=True), want_ps)):
        assert engine.store_take_compact(np.arange(nq))[1].size == nc and engine.held_cols == nc
        with pytest.raises(ValueError):
            call(H[cols])
        assert engine.held_cols == nc                                           # (refused before anything ran)
        _eq(call(H)["out64"], want, "propagate over a compacted result")
        assert engine.get_option("sparse_cols") == n
    # a new take: n columns again, [n, d] operands, the bits of before
    rp2, _ = engine.store_take(np.arange(nq))
    _eq(rp2, row_ptr, "row_ptr")
    assert engine.get_option("sparse_cols") == n == engine.held_cols
    assert _raw_cols_fetch(engine, np.zeros(n, np.int32), n) == E_ARG
    _eq(_fetch(engine, e)[0], ids, "ids")
    _eq(engine.sparse_propagate(rp2, H, want64=True)[1], before, "propagate")
    with pytest.raises(ValueError):
        engine.sparse_propagate(rp2, H[cols], want64=True)
    # an empty held result compacts to no columns, and a product over it is zeros
    live = pick_sources(g, 2, 9502)             # (no entry of a live source's row reaches 1.0: two empty rows)
    for make in (lambda: engine.store_take([])[0], lambda: engine.query_sparse(live, threshold=1.0)[0]):
        rp0 = make()
        assert int(rp0[-1]) == 0
        cols0, st0 = engine.sparse_compact(rp0)
        assert cols0.size == 0 and cols0.dtype == np.int32 and (st0["entries"], st0["cols"], st0["words"]) == (0, 0, 0)
        assert engine.get_option("sparse_cols") == 0
        assert _raw_cols_fetch(engine, None, 0) == 0
        out = engine.sparse_propagate(rp0, np.zeros((0, 3), np.float32), want64=True)[1]
        assert out.shape == (rp0.size - 1, 3) and (_bits(out) == 0).all()
        if rp0.size > 1:
            out_t = engine.sparse_propagate_t(rp0, np.ones((rp0.size - 1, 3), np.float32), want64=True)[1]
            assert out_t.shape == (0, 3)
        assert _raw_compact(engine, rp0, rp0.size - 1, one) == E_ARG              # compacted already, with nc == 0
    # sparse_clear and set_graph leave nothing behind
    for drop in (engine.sparse_clear, lambda: _load(engine, g, epsilon=0.5)):
        engine.store_put(engine.query_sparse_topk(srcs, 32, threshold=0.0)[0])
        rp, cols3, _ = engine.store_take_compact(np.arange(nq))
        _eq(cols3, cols, "cols")
        assert engine.held_cols == nc
        drop()
        assert engine.get_option("sparse_cols") == n
        assert _raw_cols_fetch(engine, np.zeros(n, np.int32), n) == E_ARG
        assert _raw_compact(engine, rp, nq, one) == E_ARG
    assert engine.store_info() == {"rows": 0, "entries": 0, "max_row": 0}       # (set_graph dropped the store too)
    _eq(engine.sparse_propagate(engine.query_sparse_topk(srcs, 32, threshold=0.0)[0], H, want64=True)[1], before, "propagate")
    # a NULL ctx is answered by both entry points
    assert lib.fora_hip_sparse_compact(None, _p(one), C.c_int(0), _p(one), None) == E_ARG
    assert lib.fora_hip_sparse_cols_fetch(None, None, C.c_uint64(0)) == E_ARG


def test_device_tensors_and_autograd():
    """store_take_compact(device=True) and the torch_ops functions over X[cols], in a child of their own
    (tests/cols_device_child.py): torch and the library must live on one HIP runtime, so the child imports torch first."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "cols_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "cols device ok" in r.stdout
