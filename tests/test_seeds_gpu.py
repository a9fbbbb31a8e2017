"""Seed sets on the GPU (fora_hip_query_seeds_batch, Engine.query_seeds): PPR restarting on weighted sets of nodes, the rows
of the seeds combined on the device.  The expected rows never pass through the new code: they are the Engine.query_fix rows
of the individual seeds (pinned to oracle/fora_twin.c by test_hip_parity_gpu.py) folded by tests/seeds_ref.py in Python
ints."""
import ctypes as C

import numpy as np
import pytest

import seeds_ref as sr
from conftest import pick_sources
from fora_amd import ForaError, synth

pytestmark = pytest.mark.gpu
SEED = 0x464F5241
ALPHA = 0.2
EPS = 0.5


def _load(engine, g):
    engine.clear_index()
    engine.reset_options()
    engine.set_batch(0)
    engine.set_balanced(False)
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(alpha=ALPHA, epsilon=EPS, seed=SEED)


@pytest.fixture(scope="module")
def odd(oracle):
    """n odd: every other row of the slabs and of the accumulator block starts at an odd word (no 16-byte alignment)."""
    src, dst = synth.rmat_graph(1999, 16000, 20260118)
    return oracle.Graph.from_edges(1999, 16000, src, dst)


def _sets(g):
    """The sets of one call, and a weight list of the same shape for the weighted call."""
    live = [int(x) for x in pick_sources(g, 16, 601)]
    dang = [int(x) for x in pick_sources(g, 2, 602, want_dangling=True)]
    sets = [
        [live[0]],                                      # a singleton: the query_fix row, word for word
        [live[1], live[2], live[3]],                    # 2^62 mod 3 != 0
        [live[4], live[5], live[4]] + dang[:1],         # a duplicate seed and, where there is one, a dangling seed
        [live[0], live[1], live[2], live[3], live[14]],  # two sets sharing most seeds
        [live[0], live[1], live[2], live[3], live[15]],
        [live[1], live[2], live[3]],                    # a duplicate of set 1
        live[3:14],                                     # 11 seeds: three batches at set_batch(4), other sets start mid-batch
    ]
    if dang:
        sets.insert(3, [dang[0], dang[-1], dang[0]])    # only dangling seeds
    rng = np.random.Generator(np.random.PCG64(603))
    weights = [[float(x) for x in rng.integers(1, 1000, size=len(s)) / 64.0] for s in sets]
    weights[0] = [0.3]                                  # one weight that is the whole sum
    weights[2] = [0.5, 1.25, 2.0, 0.75][:len(sets[2])]
    weights[-1][4] = 0.0                                # a zero weight among others
    return sets, weights


_REF = {}


def _reference(engine, g, with_idx=False):
    """Per graph, once: the sets, the query_fix rows of their seeds as Python ints, and the expected rows / top-k inputs of
    the uniform and of the weighted call.  The engine must be loaded with g (and hold its index for with_idx)."""
    key = (id(g), with_idx)
    if key not in _REF:
        sets, weights = _sets(g)
        distinct = sorted({s for st in sets for s in st})
        fix, _, _ = engine.query_fix(np.array(distinct, dtype=np.int32), with_idx=with_idx, want_residue=False)
        rows = {s: fix[i].tolist() for i, s in enumerate(distinct)}
        for s in distinct:
            if g.deg[s] == 0:
                assert rows[s][s] == sr.ONE and sum(rows[s]) == sr.ONE
        wu = [sr.uniform_wfix(len(st)) for st in sets]
        ww = [sr.weighted_wfix(w) for w in weights]
        exp_u = [sr.combine([rows[s] for s in st], w) for st, w in zip(sets, wu)]
        exp_w = [sr.combine([rows[s] for s in st], w) for st, w in zip(sets, ww)]
        _REF[key] = (g, sets, weights, rows, (wu, exp_u), (ww, exp_w))
    return _REF[key][1:]


def _counts(g, sets, dedup):
    listed = [s for st in sets for s in st]
    live = [s for s in listed if g.deg[s] > 0]
    return dict(seeds=len(listed), distinct=len(set(listed)), dangling=len(listed) - len(live),
                queries=len(set(live)) if dedup else len(live))


def _check_call(engine, g, sets, weights, wfix, expect, dedup, with_idx=False, full=False):
    out = engine.query_seeds(sets, weights=weights, with_idx=with_idx, want_ppr=full)
    fix, st = out["fix"], out["stats"]
    assert fix.shape == (len(sets), g.n) and fix.dtype == np.uint64
    for i, want in enumerate(expect):
        got = fix[i].tolist()
        if got != want:
            bad = [v for v in range(g.n) if got[v] != want[v]]
            raise AssertionError(f"set {i} {sets[i]}: {len(bad)} words differ, first at node {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")
        assert int(out["row_sum_fix"][i]) == sum(want) <= sum(wfix[i])
    for name, want in _counts(g, sets, dedup).items():
        assert st[name] == want, name
    assert st["batches"] >= 1 and st["combine_ms"] >= 0
    if full:
        assert out["ppr"].dtype == np.float64
        assert np.array_equal(out["ppr"], np.ldexp(fix.astype(np.float64), -62))
    return out


def _config(engine, batch=0, dedup=1, wide=False):
    if wide:
        engine.set_option("force_wide", 1)  # the option tests/test_hip_parity_gpu.py forces the wide layout with
    engine.set_option("seeds_dedup", dedup)
    engine.set_batch(batch)


@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling", "odd", "small"])
def test_rows_equal_the_combined_query_fix_rows(engine, request, gname):
    g = request.getfixturevalue(gname)
    _load(engine, g)
    sets, weights, rows, (wu, exp_u), (ww, exp_w) = _reference(engine, g)
    try:
        out = _check_call(engine, g, sets, None, wu, exp_u, dedup=1, full=True)
        assert out["fix"][0].tolist() == rows[sets[0][0]]            # the singleton: x unchanged
        assert np.array_equal(out["fix"][1], out["fix"][-2])         # duplicate sets give duplicate rows
        out = _check_call(engine, g, sets, weights, ww, exp_w, dedup=1, full=True)
        assert out["fix"][0].tolist() == rows[sets[0][0]]            # a weight equal to the whole sum: 2^62
        flat = (np.cumsum([0] + [len(s) for s in sets]), np.concatenate(sets))  # the (set_ptr, seeds) form, flat weights
        again = engine.query_seeds(flat, weights=np.concatenate(weights))
        assert np.array_equal(again["fix"], out["fix"])
    finally:
        engine.reset_options()


@pytest.mark.parametrize("gname", ["tiny_dangling", "odd"])
@pytest.mark.parametrize("batch,dedup,wide", [(4, 1, False), (1, 1, False), (4, 0, False), (0, 0, False), (0, 1, True), (4, 0, True)])
def test_same_bits_whatever_the_batching_dedup_and_layout(engine, request, gname, batch, dedup, wide):
    g = request.getfixturevalue(gname)
    _load(engine, g)
    sets, weights, rows, (wu, exp_u), (ww, exp_w) = _reference(engine, g)
    try:
        _config(engine, batch, dedup, wide)
        out = _check_call(engine, g, sets, None, wu, exp_u, dedup)
        _check_call(engine, g, sets, weights, ww, exp_w, dedup)
        if batch == 4:
            assert out["stats"]["batches"] == -(-out["stats"]["queries"] // 4) >= 3
        if batch == 1:
            assert out["stats"]["batches"] == out["stats"]["queries"]
    finally:
        engine.reset_options()
        engine.set_batch(0)


@pytest.mark.parametrize("batch", [0, 4])
def test_with_idx_rows_come_from_the_indexed_queries(engine, tiny_dangling, batch):
    g = tiny_dangling
    _load(engine, g)
    try:
        engine.build_index()
        sets, weights, rows, (wu, exp_u), (ww, exp_w) = _reference(engine, g, with_idx=True)
        _config(engine, batch)
        _check_call(engine, g, sets, None, wu, exp_u, 1, with_idx=True)
        _check_call(engine, g, sets, weights, ww, exp_w, 1, with_idx=True)
    finally:
        engine.reset_options()
        engine.set_batch(0)
        engine.clear_index()


@pytest.mark.parametrize("gname", ["tiny_dangling", "odd"])
def test_topk_of_the_set_rows(engine, request, gname):
    g = request.getfixturevalue(gname)
    _load(engine, g)
    sets, weights, rows, (wu, exp_u), _ = _reference(engine, g)
    for k in (1, 5, min(1024, g.n)):
        out = engine.query_seeds(sets, k=k, want_fix=False)
        assert out["fix"] is None and out["ppr"] is None and out["ids"].shape == (len(sets), k)
        for i, want in enumerate(exp_u):
            ids, sc = sr.topk(want, k)
            assert out["ids"][i].tolist() == ids, (k, i)
            assert out["scores"][i].tolist() == sc, (k, i)
    if gname == "tiny_dangling":  # rows of few non-zero words: padding
        i = 3
        assert all(g.deg[s] == 0 for s in sets[i])
        assert out["ids"][i].tolist()[2:] == [0] * (k - 2) and out["scores"][i].tolist()[2:] == [0.0] * (k - 2)
    try:
        for batch, compact in ((2, -1), (0, 1), (3, 1)):
            engine.set_batch(batch)  # fewer slots than rows: the select goes over the block in chunks
            engine.set_option("select_compact", compact)  # 1: the select of large graphs, over the block's compacted non-zeros
            out = engine.query_seeds(sets, k=5, want_fix=False)
            for i, want in enumerate(exp_u):
                assert (out["ids"][i].tolist(), out["scores"][i].tolist()) == sr.topk(want, 5), (batch, compact, i)
    finally:
        engine.reset_options()
        engine.set_batch(0)


def test_weights_mean_what_they_say(engine, tiny):
    """Semantics, independent of the fixed-point formula.  With exact rows P_j (Engine.power_iteration) and E = sum_j w_j P_j
    in doubles, the triangle inequality for a convex combination gives
        max|ppr_g - E| <= max_j max|x_j * 2^-62 - P_j| + slack,
    the first term measured here from existing entry points.  slack covers, per term, the floor of the term and the floor of
    wfix (one unit of 2^-62 each, the row words being <= 1) and the roundings of w_j / S, of the product and of the add in E
    (2^-53 each on values <= 1), plus the rounding of ppr_g itself: 2 k 2^-62 + (3 k + 1) 2^-53.  A mis-normalised or
    mis-indexed weight misses the bound by orders of magnitude."""
    g = tiny
    _load(engine, g)
    sets, weights, rows, _, _ = _reference(engine, g)
    distinct = sorted(rows)
    P, _, _, _ = engine.power_iteration(np.array(distinct, dtype=np.int32))
    P = {s: P[i] for i, s in enumerate(distinct)}
    err = {s: float(np.abs(np.ldexp(np.array(rows[s], dtype=np.uint64).astype(np.float64), -62) - P[s]).max()) for s in distinct}
    for w in (None, weights):
        out = engine.query_seeds(sets, weights=w, want_ppr=True)
        for i, st in enumerate(sets):
            k = len(st)
            S = 0.0
            for x in (w[i] if w is not None else []):
                S += x  # left to right, as the contract adds it
            wi = [1.0 / k] * k if w is None else [x / S for x in w[i]]
            E = np.zeros(g.n)
            for s, x in zip(st, wi):
                E += x * P[s]
            bound = max(err[s] for s in st) + 2 * k * 2.0 ** -62 + (3 * k + 1) * 2.0 ** -53
            got = float(np.abs(out["ppr"][i] - E).max())
            print(f"set {i} (k = {k}, {'uniform' if w is None else 'weighted'}): max|ppr - E| = {got:.3e}, bound {bound:.3e}")
            assert got <= bound, i
            if k > 1:  # the bound is sharp enough to see a wrong weight: the first seed's weight given to the second
                wrong = np.zeros(g.n)
                for s, x in zip(st, wi[1:] + wi[:1]):
                    wrong += x * P[s]
                if len(set(st)) > 1 and len(set(wi)) > 1:
                    assert float(np.abs(out["ppr"][i] - wrong).max()) > bound


def _raw(engine, set_ptr, seeds, weights, ns, with_idx=0, k=0):
    lib = engine._lib
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return lib.fora_hip_query_seeds_batch(engine._ctx, p(set_ptr), p(seeds), p(weights), C.c_int(ns), C.c_int(with_idx), None, None,
                                          C.c_int(k), None, None, None, None)


def test_argument_errors_leave_the_engine_as_it_was(engine, tiny):
    g = tiny
    _load(engine, g)
    probe = pick_sources(g, 2, 604)
    base, _ = engine.query(probe)
    a, b = int(probe[0]), int(probe[1])
    i64 = lambda *x: np.array(x, dtype=np.int64)
    i32 = lambda *x: np.array(x, dtype=np.int32)
    f64 = lambda *x: np.array(x, dtype=np.float64)
    kmax = min(1024, g.n)
    cases = {
        "ns < 0": (i64(0, 1), i32(a), None, -1, 0, 0),
        "null set_ptr": (None, i32(a), None, 1, 0, 0),
        "null seeds": (i64(0, 1), None, None, 1, 0, 0),
        "set_ptr[0] != 0": (i64(1, 2), i32(a, b), None, 1, 0, 0),
        "decreasing set_ptr": (i64(0, 2, 1), i32(a, b), None, 2, 0, 0),
        "empty set": (i64(0, 0, 1), i32(a), None, 2, 0, 0),
        "seed == n": (i64(0, 2), i32(a, g.n), None, 1, 0, 0),
        "seed < 0": (i64(0, 2), i32(-1, a), None, 1, 0, 0),
        "negative weight": (i64(0, 2), i32(a, b), f64(1.0, -0.5), 1, 0, 0),
        "nan weight": (i64(0, 2), i32(a, b), f64(1.0, float("nan")), 1, 0, 0),
        "inf weight": (i64(0, 2), i32(a, b), f64(float("inf"), 1.0), 1, 0, 0),
        "zero sum": (i64(0, 1, 3), i32(a, a, b), f64(1.0, 0.0, 0.0), 2, 0, 0),
        "with_idx without an index": (i64(0, 1), i32(a), None, 1, 1, 0),
        "k < 0": (i64(0, 1), i32(a), None, 1, 0, -1),
        "k > min(1024, n)": (i64(0, 1), i32(a), None, 1, 0, kmax + 1),
    }
    for name, (set_ptr, seeds, weights, ns, with_idx, k) in cases.items():
        assert _raw(engine, set_ptr, seeds, weights, ns, with_idx, k) == -1, name  # FORA_E_ARG
        again, _ = engine.query(probe)
        assert np.array_equal(again, base), name
    with pytest.raises(ForaError) as e:  # ... and through the binding
        engine.query_seeds([[a], []])
    assert e.value.code == -1
    with pytest.raises(ValueError):
        engine.query_seeds([[a, b]], weights=[[1.0]])
    assert _raw(engine, i64(0, 1), i32(a), None, 1, 0, kmax) == 0  # the largest k is fine


def test_empty_call(engine, tiny):
    _load(engine, tiny)
    out = engine.query_seeds([], k=3, want_ppr=True)
    assert out["fix"].shape == (0, tiny.n) and out["ppr"].shape == (0, tiny.n) and out["ids"].shape == (0, 3)
    assert out["row_sum_fix"].size == 0
    assert all(v == 0 for v in out["stats"].values())
    assert _raw(engine, None, None, None, 0) == 0  # nothing to read: null arrays are fine


def test_a_held_sparse_result_survives(engine, tiny_dangling):
    g = tiny_dangling
    _load(engine, g)
    sets, weights, rows, (wu, exp_u), _ = _reference(engine, g)
    srcs = np.array(sets[-1][:5] + sets[3][:1], dtype=np.int32)
    row_ptr, ids, vals, fix, _, sp = engine.query_sparse(srcs, want_fix=True)
    e = int(sp["entries"])
    assert e == ids.size > 0
    _check_call(engine, g, sets, None, wu, exp_u, 1)

    def fetch():
        i2, v2, f2 = np.zeros(e, dtype=np.int32), np.zeros(e, dtype=np.float64), np.zeros(e, dtype=np.uint64)
        engine.sparse_fetch(i2, v2, f2, cap=e)
        return i2, v2, f2
    for x, y in zip(fetch(), (ids, vals, fix)):
        assert np.array_equal(x, y)
    engine.sparse_clear()


@pytest.mark.parametrize("batch", [0, 4])
def test_timing_folds_the_underlying_queries(engine, tiny_dangling, batch):
    """fora_timing advances by what the same distinct seeds cost through engine.query: as many batches, the same pops,
    relaxations and walks."""
    g = tiny_dangling
    _load(engine, g)
    sets, _, _, _, _ = _reference(engine, g)
    order = list(dict.fromkeys(s for st in sets for s in st if g.deg[s] > 0))  # the slots: first appearance
    engine.set_batch(batch)
    try:
        engine.query(np.array(order, dtype=np.int32), want_ppr=False)  # (the workspace is planned)
        engine.reset_timing()
        engine.query(np.array(order, dtype=np.int32), want_ppr=False)
        t1 = engine.timing()
        engine.reset_timing()
        out = engine.query_seeds(sets, want_fix=False)
        t2 = engine.timing()
    finally:
        engine.set_batch(0)
    for name in ("batches", "pops", "relax", "walks", "walk_steps", "idx_hits"):
        assert t2[name] == t1[name], name
    assert t1["batches"] == out["stats"]["batches"] and t1["pops"] > 0
    assert out["stats"]["queries"] == len(order)
