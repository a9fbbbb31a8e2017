"""SUBGRAPH PRODUCTS on the GPU, through the C ABI (the contract of include/fora_hip_gnn.h): out = A_S x X and out = A_S^T x G over
the held subgraph are the numpy twin's (tests/subgraph_prop_ref.py) bit for bit, under every value of "sub_short", "prop_segs"
and "propt_lds_cap", with unit weights, f32 and f64 values, MEAN and every element type; the transposition is the twin's stable
order; the calls leave the held result and the subgraph as they were -- every comparison here is an equality of bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import narrow_ref
import propagate_ref as pr
import propagate_values_ref as pv
import subgraph_prop_ref as sr
import subgraph_ref
from conftest import pick_sources
from test_sparse_gpu import _load

pytestmark = pytest.mark.gpu
E_ARG = -1
DS = [1, 3, 8, 33, 64]
# (sub_short, prop_segs, propt_lds_cap): the defaults; both paths with the long one in several chunks; the long path alone, in
# chunks of one segment, the transposition's runs sorted on the global tier
CONFIGS = [(None, None, None), (64, 2, None), (0, 1, 0)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _eq(a, b, name):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    assert (a.view(np.uint8) == b.view(np.uint8)).all(), name


class Crafted:
    """an Engine of its own over the crafted graph (the session engine's graph is untouched); row 0 of its store is U, row 1 two
    nodes without an edge between them"""

    def __init__(self):
        import fora_amd
        self.row_ptr, self.col, self.U = sr.crafted_graph()
        self.sub = subgraph_ref.induced(self.row_ptr, self.col, self.U)
        self.eng = fora_amd.Engine(0)
        self.eng.set_graph(sr.CRAFTED_N, int(self.row_ptr[-1]), self.row_ptr, self.col)
        ids = np.concatenate([self.U, [0, 721]]).astype(np.int32)
        self.eng.store_load(np.array([0, self.U.size, ids.size], dtype=np.int64), ids, np.full(ids.size, 1 << 40, dtype=np.uint64))

    def take(self, config=(None, None, None), row=0):
        """the options of a config, then the subgraph built again under them (the transposition is built with it)"""
        self.eng.reset_options()
        for name, v in zip(("sub_short", "prop_segs", "propt_lds_cap"), config):
            if v is not None:
                self.eng.set_option(name, v)
        return self.eng.store_take_subgraph([row, row])


@pytest.fixture(scope="module")
def crafted():
    c = Crafted()
    sub_ptr, sub_col = c.sub[0], c.sub[1]
    assert sorted(np.diff(sub_ptr)[1:11].tolist()) == sr.LENS and np.diff(sub_ptr)[[0, 721]].tolist() == [0, 0]
    assert np.bincount(sub_col, minlength=sr.CRAFTED_NC)[11:21].tolist() == sr.LENS
    assert sub_col[sub_ptr[3]] == sub_col[sub_ptr[3] + 1] and 21 in sub_col[sub_ptr[21]:sub_ptr[22]]   # the duplicate pair, the self-loop
    yield c
    c.eng.close()


@pytest.fixture(scope="module")
def operands(crafted):
    """X [nc, 64] and one value per edge, all different and scaled over 2^+-20: a wrong order or place changes bits"""
    rng = np.random.Generator(np.random.PCG64(9900))
    edges = crafted.sub[1].size
    return {"X": pv.distinct_values(rng, sr.CRAFTED_NC * 64, np.float32).reshape(sr.CRAFTED_NC, 64),
            "v32": pv.distinct_values(rng, edges, np.float32), "v64": pv.distinct_values(rng, edges, np.float64)}


@pytest.mark.parametrize("d", DS)
def test_both_directions_against_the_twin_under_every_option(crafted, operands, d):
    eng, (sub_ptr, sub_col, _, _) = crafted.eng, crafted.sub
    X = np.ascontiguousarray(operands["X"][:, :d])
    weights = {"unit": None, "f32": operands["v32"], "f64": operands["v64"]}
    want = {(t, w): (sr.propagate_t if t else sr.propagate)(sub_ptr, sub_col, X, values=v) for t in (False, True) for w, v in weights.items()}
    try:
        for config in CONFIGS:
            crafted.take(config)
            for (t, w), (w64, w32) in want.items():
                fn = eng.subgraph_propagate_t if t else eng.subgraph_propagate
                o32, o64, st = fn(X, values=weights[w], want32=True, want64=True)
                _eq(o64, w64, f"out64 {config} transposed={t} {w}")
                _eq(o32, w32, f"out32 {config} transposed={t} {w}")
                cap = 256 if config[0] is None else config[0]
                lens = np.bincount(sub_col, minlength=sr.CRAFTED_NC) if t else np.diff(sub_ptr)
                assert st["long_rows"] == int((lens > cap).sum()) and st["x_on_device"] == 0 and st["edges"] == sub_col.size, (config, st)
                if config[1] is not None:
                    assert st["chunks"] == -(-int(((lens[lens > cap] + 255) // 256).sum()) // config[1]) > 1, (config, st)
    finally:
        eng.reset_options()


@pytest.mark.parametrize("d", [3, 33])
def test_mean_and_mean_with_values_refused(crafted, operands, d):
    eng, (sub_ptr, sub_col, _, _) = crafted.eng, crafted.sub
    X = np.ascontiguousarray(operands["X"][:, :d])
    want = {t: (sr.propagate_t if t else sr.propagate)(sub_ptr, sub_col, X, mean=True) for t in (False, True)}
    try:
        for config in CONFIGS:
            crafted.take(config)
            for t, (w64, w32) in want.items():
                o32, o64, _ = (eng.subgraph_propagate_t if t else eng.subgraph_propagate)(X, mean=True, want32=True, want64=True)
                _eq(o64, w64, f"mean out64 {config} transposed={t}")
                _eq(o32, w32, f"mean out32 {config} transposed={t}")
                assert not np.signbit(o64[[0, 721]]).any() and not o64[[0, 721]].any()           # rows without terms: +0.0
    finally:
        eng.reset_options()
    out = np.full((sr.CRAFTED_NC, d), np.nan, dtype=np.float32)
    for fn in (eng._lib.fora_hip_subgraph_propagate, eng._lib.fora_hip_subgraph_propagate_t):
        assert fn(eng._ctx, _p(X), 0, d, d, 1, _p(operands["v32"]), 0, _p(out), None, d, None, None) == E_ARG
        assert fn(eng._ctx, _p(X), 0, d, d, 2, None, 0, _p(out), None, d, None, None) == E_ARG    # another flag bit
    assert np.isnan(out).all()
    with pytest.raises(Exception):
        eng.subgraph_propagate(X, values=operands["v32"], mean=True)


@pytest.mark.parametrize("kind", ["bf16", narrow_ref.F16, narrow_ref.E4M3, narrow_ref.E5M2])
def test_narrow_operands_against_the_widened_f32_call(crafted, kind):
    eng, d = crafted.eng, 32
    rng = np.random.Generator(np.random.PCG64(9910))
    crafted.take((64, 2, None))
    try:
        if kind == "bf16":
            codes = pr.to_bf16_bits(pv.distinct_values(rng, sr.CRAFTED_NC * d, np.float32).reshape(sr.CRAFTED_NC, d))
            operand, keyword = codes, True
        else:
            codes = narrow_ref.moderate_codes(rng, kind, (sr.CRAFTED_NC, d))
            operand, keyword = narrow_ref.as_operand(kind, codes)
        wide = sr.widen32(codes, kind)
        for fn in (eng.subgraph_propagate, eng.subgraph_propagate_t):
            got = fn(operand, bf16=keyword, want32=True, want64=True)
            ref = fn(wide, want32=True, want64=True)
            _eq(got[0], ref[0], f"{kind} out32")
            _eq(got[1], ref[1], f"{kind} out64")
            assert got[1].any()
    finally:
        eng.reset_options()


def test_outputs_alone_and_together_and_the_transposition(crafted, operands):
    eng, (sub_ptr, sub_col, _, _) = crafted.eng, crafted.sub
    crafted.take()
    X = np.ascontiguousarray(operands["X"][:, :8])
    in_ptr, in_row, in_pos = eng.subgraph_transpose_fetch()                      # builds it
    for a, b, name in zip((in_ptr, in_row, in_pos), sr.transpose(sub_ptr, sub_col), ("in_ptr", "in_row", "in_pos")):
        _eq(a, b, name)
    for fn in (eng.subgraph_propagate, eng.subgraph_propagate_t):
        b32, b64, st = fn(X, want32=True, want64=True)
        assert st["built"] == 0                                                  # (the fetch built it; a later call never does)
        o32, none, _ = fn(X, want32=True, want64=False)
        assert none is None
        _eq(o32, b32, "out32 alone")
        none, o64, _ = fn(X, want32=False, want64=True)
        assert none is None
        _eq(o64, b64, "out64 alone")
        wide32, wide64 = np.full((sr.CRAFTED_NC, 11), 7.0, np.float32), np.full((sr.CRAFTED_NC, 11), 7.0, np.float64)
        fn(X, out32=wide32[:, :8], out64=wide64[:, :8])                           # a pitch of the caller's: the columns behind d stay
        _eq(wide32[:, :8], b32, "out32 at a pitch")
        _eq(wide64[:, :8], b64, "out64 at a pitch")
        assert (wide32[:, 8:] == 7.0).all() and (wide64[:, 8:] == 7.0).all()
    crafted.take()                                                               # built again: the first transposed call builds, the second does not
    assert eng.subgraph_propagate(X)[2]["built"] == 0
    assert eng.subgraph_propagate_t(X)[2]["built"] == 1 and eng.subgraph_propagate_t(X)[2]["built"] == 0


def test_lifetime_errors_and_what_the_calls_leave_alone(crafted, operands):
    eng, lib = crafted.eng, crafted.eng._lib
    d = 3
    X = np.ascontiguousarray(operands["X"][:, :d])
    out = np.full((sr.CRAFTED_NC, d), np.nan, dtype=np.float32)
    raw = lambda fn, x=X, xt=0, dd=d, o32=out, o64=None: fn(eng._ctx, _p(x), xt, dd, max(dd, 1), 0, None, 0, _p(o32), _p(o64), max(dd, 1), None, None)
    fns = (lib.fora_hip_subgraph_propagate, lib.fora_hip_subgraph_propagate_t)
    row_ptr, cols, sub_ptr, sub_col, sub_eid, _ = eng.store_take_subgraph([0, 0], want_eid=True)
    # ---- bad arguments write nothing
    for fn in fns:
        assert raw(fn, xt=3) == E_ARG and raw(fn, xt=7) == E_ARG and raw(fn, dd=0) == E_ARG and raw(fn, o32=None) == E_ARG
        assert fn(eng._ctx, _p(X), 0, d, d - 1, 0, None, 0, _p(out), None, d, None, None) == E_ARG           # a pitch below d
        assert fn(eng._ctx, _p(X), 0, d, d, 0, _p(operands["v32"]), 1, _p(out), None, d, None, None) == E_ARG  # values of type bf16
    assert np.isnan(out).all()
    # ---- the calls leave the held result, its transposition and the subgraph as they were
    G = np.ones((2, d), dtype=np.float32)
    assert eng.sparse_propagate_t(row_ptr, G)[2]["built"] == 1
    e = int(row_ptr[-1])
    ids, fix = np.zeros(e, np.int32), np.zeros(e, np.uint64)
    eng.sparse_fetch(ids, None, fix, cap=e)
    gen, timing = eng.get_option("sparse_generation"), eng.timing()
    for fn in (eng.subgraph_propagate, eng.subgraph_propagate_t):
        fn(X, want64=True)
        fn(X, values=operands["v64"])
        fn(X, mean=True)
    assert eng.get_option("sparse_generation") == gen and eng.timing() == timing and eng.held_cols == sr.CRAFTED_NC
    ids2, fix2 = np.zeros(e, np.int32), np.zeros(e, np.uint64)
    eng.sparse_fetch(ids2, None, fix2, cap=e)
    _eq(ids2, ids, "held ids")
    _eq(fix2, fix, "held words")
    assert eng.sparse_propagate_t(row_ptr, G)[2]["built"] == 0
    again = eng.sparse_subgraph(row_ptr, want_eid=True)
    for a, b, name in zip(again[:3], (sub_ptr, sub_col, sub_eid), ("sub_ptr", "sub_col", "sub_eid")):
        _eq(a, b, name)
    for a, b in zip(again[:2], crafted.sub[:2]):
        _eq(a, b, "the twin's subgraph")
    # ---- a subgraph of 0 edges: every output row is written as +0.0
    crafted.take(row=1)
    assert eng.get_option("sub_edges") == 0 and eng.held_cols == 2
    for fn in (eng.subgraph_propagate, eng.subgraph_propagate_t):
        for mean in (False, True):
            o32, o64 = np.full((2, d), np.nan, np.float32), np.full((2, d), np.nan, np.float64)
            fn(X[:2], mean=mean, out32=o32, out64=o64)
            assert not o32.any() and not o64.any() and not np.signbit(o32).any() and not np.signbit(o64).any()
    assert eng.subgraph_transpose_fetch()[0].tolist() == [0, 0, 0]
    # ---- it ends with the held result: a compacted result without a subgraph, a new take, a clear, set_graph
    eng.store_take_compact([0, 0])
    assert eng.get_option("sub_edges") == -1
    assert all(raw(fn) == E_ARG for fn in fns) and lib.fora_hip_subgraph_transpose_fetch(eng._ctx, None, None, None, 1 << 30) == E_ARG
    with pytest.raises(Exception):
        eng.subgraph_propagate(X)
    drops = (lambda: eng.store_take([0]), eng.sparse_clear, lambda: eng.set_graph(sr.CRAFTED_N, int(crafted.row_ptr[-1]), crafted.row_ptr, crafted.col))
    for drop in drops:
        eng.store_take_subgraph([0, 0])
        assert all(raw(fn) == 0 for fn in fns) and not np.isnan(out).any()
        out[:] = np.nan
        drop()
        assert all(raw(fn) == E_ARG for fn in fns) and np.isnan(out).all()
        assert lib.fora_hip_subgraph_transpose_fetch(eng._ctx, None, None, None, 1 << 30) == E_ARG
    # (set_graph emptied the store: the fixture's later users get it back)
    ids = np.concatenate([crafted.U, [0, 721]]).astype(np.int32)
    eng.store_load(np.array([0, crafted.U.size, ids.size], dtype=np.int64), ids, np.full(ids.size, 1 << 40, dtype=np.uint64))
    # a NULL ctx is answered by all three entry points
    assert all(fn(None, _p(X), 0, d, d, 0, None, 0, _p(out), None, d, None, None) == E_ARG for fn in fns)
    assert lib.fora_hip_subgraph_transpose_fetch(None, None, None, None, 0) == E_ARG


def test_a_real_topk_result_and_a_result_without_columns(engine, small):
    g = small
    _load(engine, g, epsilon=0.5)
    srcs = pick_sources(g, 6, 9920)
    row_ptr = engine.query_sparse_topk(srcs, 16, threshold=0.0)[0]
    cols, _ = engine.sparse_compact(row_ptr)
    sub_ptr, sub_col, _, st = engine.sparse_subgraph(row_ptr)
    assert st["edges"] > 0
    rng = np.random.Generator(np.random.PCG64(9921))
    X = pv.distinct_values(rng, cols.size * 8, np.float32).reshape(cols.size, 8)
    for t, fn in ((False, engine.subgraph_propagate), (True, engine.subgraph_propagate_t)):
        o32, o64, _ = fn(X, want32=True, want64=True)
        w64, w32 = (sr.propagate_t if t else sr.propagate)(sub_ptr, sub_col, X)
        _eq(o64, w64, f"out64 transposed={t}")
        _eq(o32, w32, f"out32 transposed={t}")
        assert o64.any()
    for a, b in zip(engine.subgraph_transpose_fetch(), sr.transpose(sub_ptr, sub_col)):
        _eq(a, b, "the transposition")
    # nc = 0: FORA_OK, nothing launched, nothing to write
    rp0 = engine.query_sparse(srcs[:2], threshold=1.0)[0]
    assert int(rp0[-1]) == 0 and engine.sparse_compact(rp0)[0].size == 0
    assert engine.sparse_subgraph(rp0)[3]["edges"] == 0
    for fn in (engine.subgraph_propagate, engine.subgraph_propagate_t):
        o32, o64, st = fn(np.zeros((0, 4), np.float32), want32=True, want64=True)
        assert o32.shape == o64.shape == (0, 4) and st["built"] == 0
    assert engine.subgraph_transpose_fetch()[0].tolist() == [0]
    engine.sparse_clear()


def test_device_tensors_and_autograd():
    """Engine.subgraph_propagate over device tensors and torch_ops.subgraph_propagate, in a child of their own
    (tests/subgraph_prop_device_child.py): torch and the library must live on one HIP runtime, so the child imports torch first."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "subgraph_prop_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "subgraph products device ok" in r.stdout
