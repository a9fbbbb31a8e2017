"""SUBGRAPH on the GPU, through the C ABI (the contract of include/fora_hip_ext.h): fora_hip_sparse_subgraph builds the CSR the
graph induces on the columns of a compacted held result.  The arrays are the numpy twin's (tests/subgraph_ref.py) under every
value of "sub_span", and the call leaves the held result as it was -- every comparison here is an equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import attention_ref as ar
import subgraph_ref
from conftest import pick_sources
from test_sparse_gpu import _load, _mixed_sources

pytestmark = pytest.mark.gpu
E_ARG = -1
SPANS = [256, 1024, None]          # the minimum, a middle value, the default
N, HUB, HUB_DEG = 200, 100, 5000
EMPTY = [0, 1, 64, 129, 198, 199]  # nodes of out-degree 0


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _eq(a, b, name):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    assert (a.view(np.uint8) == b.view(np.uint8)).all(), name


def _crafted_graph():
    """200 nodes: a hub row of 5000 edges over the nodes 20 .. 59 and 126 .. 130 with duplicates and a self-loop; EMPTY without
    out-edges; the nodes 62 .. 66 point at each other, at themselves and outside; everyone else has 3 edges into 140 .. 189"""
    rng = np.random.Generator(np.random.PCG64(9700))
    rows = []
    for v in range(N):
        if v in EMPTY:
            rows.append(np.zeros(0, np.int32))
        elif v == HUB:
            t = rng.choice(np.concatenate([np.arange(20, 60), np.arange(126, 131)]), size=HUB_DEG).astype(np.int32)
            t[17] = HUB
            t[18] = t[19] = t[20]
            rows.append(t)
        elif 62 <= v <= 66:
            rows.append(np.array([v, 62 + (v - 61) % 5, 150, 62 + (v - 61) % 5, 128], dtype=np.int32))
        else:
            rows.append(rng.integers(140, 190, size=3).astype(np.int32))
    row_ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    return row_ptr, np.concatenate(rows)


@pytest.fixture(scope="module")
def crafted():
    """an Engine of its own over the crafted graph (the session engine's graph is untouched), the node sets in its row store"""
    import fora_amd
    row_ptr, col = _crafted_graph()
    hub_targets = np.setdiff1d(np.unique(col[row_ptr[HUB]:row_ptr[HUB + 1]]), [HUB])
    sets = {"every node": np.arange(N), "one node": np.array([63]), "word boundaries": np.array([62, 63, 64, 65, 66, 126, 127, 128, 129, 130]),
            "the hub alone": np.array([HUB]), "the hub's targets without the hub": hub_targets}
    eng = fora_amd.Engine(0)
    eng.set_graph(N, int(row_ptr[-1]), row_ptr, col)
    lens = [len(s) for s in sets.values()]
    ids = np.concatenate(list(sets.values())).astype(np.int32)
    eng.store_load(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), ids, np.full(ids.size, 1 << 40, dtype=np.uint64))
    yield eng, row_ptr, col, sets
    eng.close()


@pytest.mark.parametrize("which", range(5))
def test_crafted_graph_and_node_sets_under_every_span(crafted, which):
    eng, row_ptr, col, sets = crafted
    name, U = list(sets.items())[which]
    want = subgraph_ref.induced(row_ptr, col, U)
    got = []
    try:
        for span in SPANS:
            if span is None:
                eng.reset_options()
            else:
                eng.set_option("sub_span", span)
            rp, cols, sub_ptr, sub_col, sub_eid, st = eng.store_take_subgraph([which, which], want_eid=True)  # (the row twice: U is its set)
            _eq(cols, U.astype(np.int32), name + ": cols")
            _eq(sub_ptr, want[0], name + ": sub_ptr")
            _eq(sub_col, want[1], name + ": sub_col")
            _eq(sub_eid, want[2], name + ": sub_eid")
            assert (st["edges"], st["scanned"]) == (want[1].size, want[3]) and st["sub_ms"] >= 0, (name, st)
            got.append((sub_ptr, sub_col, sub_eid))
    finally:
        eng.reset_options()
    for other in got[1:]:
        for a, b in zip(got[0], other):
            _eq(a, b, name + ": across spans")
    sub_ptr, sub_col, sub_eid = got[0]
    if name == "every node":                                                   # the graph itself
        _eq(sub_col, col, "col")
        _eq(sub_eid, np.arange(col.size, dtype=np.int64), "eid")
        _eq(sub_ptr, row_ptr, "row_ptr")
    elif name == "one node":
        assert sub_col.tolist() == [0] and sub_eid.tolist() == [int(row_ptr[63])]           # its self-loop alone
    elif name == "word boundaries":
        assert np.diff(sub_ptr).tolist() == [4, 4, 0, 4, 4, 0, 0, 0, 0, 0]      # 62, 63, 65, 66 keep four of five; the rest have no in-set target or no edge
    elif name == "the hub alone":
        assert sub_col.tolist() == [0] and sub_eid.tolist() == [int(row_ptr[HUB]) + 17]     # the self-loop among 5000 scanned edges
    else:
        assert sub_col.size == 0 and st["scanned"] == 3 * (U.size - 1)          # every neighbour is outside U (129 has none)


def _held_twin(engine, g, row_ptr):
    cols, _ = engine.sparse_compact(row_ptr)
    sub_ptr, sub_col, sub_eid, st = engine.sparse_subgraph(row_ptr, want_eid=True)
    want = subgraph_ref.induced(g.row_ptr, g.col, cols)
    for a, b, name in zip((sub_ptr, sub_col, sub_eid), want, ("sub_ptr", "sub_col", "sub_eid")):
        _eq(a, b, name)
    assert (st["edges"], st["scanned"]) == (want[1].size, want[3])
    _, _, none, _ = engine.sparse_subgraph(row_ptr)                           # without the edge ids
    assert none is None
    return cols, st


def test_twin_on_topk_seed_set_and_store_results(engine, small):
    g = small
    _load(engine, g, epsilon=0.5)
    srcs = pick_sources(g, 6, 9710)
    row_ptr = engine.query_sparse_topk(srcs, 16, threshold=0.0)[0]
    engine.store_put(row_ptr)                                                   # (node ids: before the compaction)
    cols, st = _held_twin(engine, g, row_ptr)
    assert 16 <= cols.size <= 16 * len(srcs) and 0 < st["edges"] < st["scanned"]
    r = engine.query_seeds_sparse([[int(s) for s in srcs[:3]], [int(srcs[4])]])
    cols, st = _held_twin(engine, g, r["row_ptr"])
    assert cols.size > 16 and st["edges"] > 0
    row_ptr = engine.store_take([5, 0, 5, 2])[0]                                # duplicate rows
    cols, st = _held_twin(engine, g, row_ptr)
    assert 16 <= cols.size <= 48
    # a result with zero held entries has no columns and no edges, and nothing to fetch but the one offset
    rp0 = engine.query_sparse(srcs[:2], threshold=1.0)[0]
    assert int(rp0[-1]) == 0
    assert engine.sparse_compact(rp0)[0].size == 0
    sub_ptr, sub_col, sub_eid, st = engine.sparse_subgraph(rp0, want_eid=True)
    assert sub_ptr.tolist() == [0] and sub_col.size == 0 and sub_eid.size == 0 and (st["edges"], st["scanned"]) == (0, 0)
    engine.store_clear()


def test_more_rows_and_spans_than_a_scan_has_threads(engine, small):
    """n = 32 000: with every node in U the rows are 125 blocks of 256 and, at the minimum span, the scanned edges are more
    than 256 spans, so the one workgroup of the scan loops -- and the subgraph is the graph itself; with half of the nodes the
    twin decides"""
    g = small
    assert g.n == 32000 and g.col.size > 256 * 256
    _load(engine, g, epsilon=0.5)
    half = np.sort(np.random.Generator(np.random.PCG64(9730)).choice(g.n, size=g.n // 2, replace=False)).astype(np.int32)
    every = np.arange(g.n, dtype=np.int32)
    ids = np.concatenate([every, half])
    engine.store_load(np.array([0, every.size, ids.size], dtype=np.int64), ids, np.full(ids.size, 1 << 40, dtype=np.uint64))
    want_half = subgraph_ref.induced(g.row_ptr, g.col, half)
    want_every = (np.asarray(g.row_ptr, dtype=np.int64), np.asarray(g.col, dtype=np.int32), np.arange(g.col.size, dtype=np.int64), g.col.size)
    try:
        for span in (256, None):
            if span is None:
                engine.reset_options()
            else:
                engine.set_option("sub_span", span)
            for row, U, want in ((0, every, want_every), (1, half, want_half)):
                _, cols, sub_ptr, sub_col, sub_eid, st = engine.store_take_subgraph([row], want_eid=True)
                _eq(cols, U, "cols")
                for a, b, name in zip((sub_ptr, sub_col, sub_eid), want, ("sub_ptr", "sub_col", "sub_eid")):
                    _eq(a, b, name)
                assert (st["edges"], st["scanned"]) == (want[1].size, want[3])
    finally:
        engine.reset_options()
        engine.store_clear()


def _raw_build(engine, row_ptr, nq, edges):
    return engine._lib.fora_hip_sparse_subgraph(engine._ctx, _p(row_ptr), C.c_int(nq), _p(edges), None, None)


def _raw_fetch(engine, sub_ptr, sub_col, sub_eid, cap):
    return engine._lib.fora_hip_sparse_subgraph_fetch(engine._ctx, _p(sub_ptr), _p(sub_col), _p(sub_eid), C.c_uint64(cap))


def test_lifetime_errors_and_what_the_call_leaves_alone(engine, tiny_dangling):
    g = tiny_dangling
    _load(engine, g, epsilon=0.5)
    lib = engine._lib
    one = np.zeros(2, dtype=np.int64)
    srcs = _mixed_sources(g, 9720)
    nq, heads, d, dv = len(srcs), 2, 8, 6
    rng = np.random.Generator(np.random.PCG64(9721))
    engine.store_put(engine.query_sparse_topk(srcs, 32, threshold=0.0)[0])
    every = np.arange(nq)

    def held_state(row_ptr, cols):
        """everything a later call sees of the held result: the ids, the transposition, an attention over it"""
        e = int(row_ptr[-1])
        ids, fix = np.zeros(e, np.int32), np.zeros(e, np.uint64)
        engine.sparse_fetch(ids, None, fix, cap=e)
        Q, K = ar.scores_operands(np.random.Generator(np.random.PCG64(9722)), nq, g.n, d, heads, spread=6.0)
        V = np.random.Generator(np.random.PCG64(9723)).standard_normal((g.n, heads * dv)).astype(np.float32)
        o32, o64, _, y64, _ = engine.sparse_attention(row_ptr, Q, np.ascontiguousarray(K[cols]), np.ascontiguousarray(V[cols]), heads=heads,
                                                      want32=True, want64=True, want_y64=True)
        return [ids, fix, o32, o64, y64, *engine.sparse_transpose_fetch(row_ptr, want_fix=True)]

    # ---- without the call
    row_ptr, cols, _ = engine.store_take_compact(every)
    nc = cols.size
    G = rng.standard_normal((nq, 3)).astype(np.float32)
    assert engine.sparse_propagate_t(row_ptr, G, want64=True)[2]["built"] == 1
    want = held_state(row_ptr, cols)
    # ---- nothing to build on: nothing held, an uncompacted result, bad arguments
    engine.sparse_clear()
    assert _raw_build(engine, np.zeros(1, dtype=np.int64), 0, one) == E_ARG
    assert _raw_fetch(engine, None, None, None, 0) == E_ARG
    rp2 = engine.store_take(every)[0]
    _eq(rp2, row_ptr, "row_ptr")
    assert _raw_build(engine, row_ptr, nq, one) == E_ARG and "not compacted" in lib.fora_hip_last_error(engine._ctx).decode()
    with pytest.raises(Exception):
        engine.sparse_subgraph(row_ptr)
    engine.sparse_compact(row_ptr)
    assert engine.sparse_propagate_t(row_ptr, G, want64=True)[2]["built"] == 1   # the transposition, built before the subgraph is
    gen = engine.get_option("sparse_generation")
    assert _raw_fetch(engine, None, None, None, 1 << 30) == E_ARG               # compacted, but no subgraph built yet
    assert _raw_build(engine, row_ptr, nq, None) == E_ARG                       # NULL edges_out
    wrong = row_ptr.copy()
    wrong[-1] += 1
    assert _raw_build(engine, wrong, nq, one) == E_ARG and _raw_build(engine, row_ptr, nq - 1, one) == E_ARG
    assert _raw_build(engine, None, nq, one) == E_ARG
    assert _raw_fetch(engine, None, None, None, 1 << 30) == E_ARG               # (none of them left one behind)
    # ---- the build, twice
    first = engine.sparse_subgraph(row_ptr, want_eid=True)
    again = engine.sparse_subgraph(row_ptr, want_eid=True)
    edges = first[3]["edges"]
    assert edges > 0 and first[3]["scanned"] == int(np.diff(g.row_ptr)[cols].sum())
    for a, b, w in zip(first[:3], again[:3], subgraph_ref.induced(g.row_ptr, g.col, cols)):
        _eq(a, b, "a second build")
        _eq(a, w, "the twin")
    # ---- fetch: a short cap; the exact one, array by array
    sub_ptr, sub_col = np.zeros(nc + 1, np.int64), np.zeros(edges, np.int32)
    assert _raw_fetch(engine, sub_ptr, sub_col, None, edges - 1) == E_ARG
    assert not sub_ptr.any() and not sub_col.any()
    assert _raw_fetch(engine, sub_ptr, None, None, edges) == 0 and _raw_fetch(engine, None, sub_col, None, edges) == 0
    _eq(sub_ptr, first[0], "sub_ptr")
    _eq(sub_col, first[1], "sub_col")
    # ---- the held result is what it was: generation, columns, transposition (not built again), ids, words, attention
    assert engine.get_option("sparse_generation") == gen and engine.held_cols == nc == engine.get_option("sparse_cols")
    assert engine.sparse_propagate_t(row_ptr, G, want64=True)[2]["built"] == 0
    for a, b in zip(held_state(row_ptr, cols), want):
        _eq(a, b, "held state behind the call")
    assert engine.get_option("sparse_generation") == gen
    assert _raw_fetch(engine, sub_ptr, sub_col, None, edges) == 0               # ... and the calls on the held rows left the subgraph
    # ---- it ends with the held result: a new take, a clear, set_graph
    engine.store_take(every)
    assert _raw_fetch(engine, sub_ptr, sub_col, None, edges) == E_ARG
    for drop in (engine.sparse_clear, lambda: _load(engine, g, epsilon=0.5)):
        rp, _, _, _, _, st = engine.store_take_subgraph(every)
        assert st["edges"] == edges and _raw_fetch(engine, sub_ptr, sub_col, None, edges) == 0
        drop()
        assert _raw_fetch(engine, sub_ptr, sub_col, None, edges) == E_ARG
        assert _raw_build(engine, rp, nq, one) == E_ARG
    # a NULL ctx is answered by both entry points
    assert lib.fora_hip_sparse_subgraph(None, _p(one), C.c_int(0), _p(one), None, None) == E_ARG
    assert lib.fora_hip_sparse_subgraph_fetch(None, None, None, None, C.c_uint64(0)) == E_ARG


def test_device_tensors_and_edge_index():
    """store_take_subgraph(device=True) and subgraph_edge_index over tensors, in a child of their own
    (tests/subgraph_device_child.py): torch and the library must live on one HIP runtime, so the child imports torch first."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "subgraph_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "subgraph device ok" in r.stdout
