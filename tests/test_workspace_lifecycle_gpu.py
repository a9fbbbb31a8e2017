"""Life cycle of the workspace (fora_hip.hip: struct Workspace): whatever order the calls come in and however often the
workspace is re-planned between them -- a fixed batch size, back to the automatic one, a bucket retry in mid-call, another
graph and back -- every call returns the bits it returned on a fresh plan.  The lazily allocated buffers (top-k slabs,
bounds, --balanced marks, select counts) are sized by the plan they were allocated under and must follow it."""
import numpy as np
import pytest

from conftest import pick_sources

pytestmark = pytest.mark.gpu
SEED = 0x464F5241
K = 8
CALLS = ("query", "balanced", "topk", "topk_bound", "power")


def _load(engine, g):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(epsilon=0.5, seed=SEED)
    return engine.get_params()


def _call(engine, name, srcs):
    """One of the five calls; its result arrays as bytes."""
    if name == "query":
        out = engine.query_fix(srcs)[:2]
    elif name == "balanced":
        engine.set_balanced(True)
        try:
            out = engine.query_fix(srcs)[:2]
        finally:
            engine.set_balanced(False)
    elif name == "topk":
        out = engine.topk(srcs, K, epsilon=0.5)
    elif name == "topk_bound":
        out = engine.topk_bound(srcs, K, epsilon=0.5)
    else:
        _, fix, ids, sc = engine.power_iteration(srcs, max_iter=30, k=K, want_ppr=False, want_fix=True)
        out = (fix, ids, sc)
    return tuple(np.ascontiguousarray(a).tobytes() for a in out)


def _run(engine, srcs, order):
    return {name: _call(engine, name, srcs) for name in order}


def _same(got, base, leg):
    for name in CALLS:
        assert got[name] == base[name], (leg, name)


def test_results_survive_every_replan(engine, oracle, small_dangling, tiny_dangling):
    g = small_dangling
    live, dang = pick_sources(g, 6, 411), pick_sources(g, 1, 412, want_dangling=True)
    srcs = np.concatenate([live[:2], dang, live[2:]]).astype(np.int32)
    assert srcs.size == 7 and (g.deg[srcs] == 0).sum() == 1
    try:
        engine.reset_options()
        rmax, omega = _load(engine, g)
        assert engine.get_batch() == 0                      # a fresh plan
        ppr, res, st = engine.query_fix(srcs)
        for i, s in enumerate(srcs):                        # as test_query_bit_exact_vs_twin
            want, wres, wst = oracle.twin_query(g, int(s), rmax, omega, seed=SEED)
            assert (res[i] == wres).all()
            assert (ppr[i] == want).all()
            assert st[i]["n_walks"] == wst["n_walks"] and st[i]["n_idx_hit"] == 0
            assert st[i]["ppr_sum_fix"] == int(want.sum())
            if wst["rsum_fix"]:
                assert st[i]["ppr_sum_fix"] == oracle.FIX_ONE
        base = _run(engine, srcs, CALLS)
        assert base["query"] == (ppr.tobytes(), res.tobytes())

        # a: --balanced allocates its marks first, the top-k drivers their slabs after it
        engine.reset_options()
        assert engine.get_batch() == 0
        _same(_run(engine, srcs, ("balanced", "topk", "topk_bound", "query", "power")), base, "a")
        assert engine.get_batch() > 0

        # b: three slots -- batches of 3 + 3 + 1, smaller lazy buffers; the calls in reverse order
        engine.set_batch(3)
        assert engine.get_batch() == 0
        _same(_run(engine, srcs, CALLS[::-1]), base, "b")
        assert engine.get_batch() == 3

        # c: the automatic slot count again -- every buffer grows back
        engine.set_batch(0)
        assert engine.get_batch() == 0
        _same(_run(engine, srcs, CALLS), base, "c")
        assert engine.get_batch() > 3

        # d: buckets and overflow list far too small (the values of test_bucket_overflow_is_retried_with_larger_buckets):
        # the top-k call frees and re-plans the workspace between its attempts
        engine.set_option("bkcap", 8)
        engine.set_option("ovcap", 64)
        engine.set_option("tail", 0)
        assert engine.get_batch() == 0 and engine.get_option("bkcap") == 8
        r0 = engine.get_option("bucket_retries")
        got = _run(engine, srcs, ("topk",))
        assert engine.get_option("bucket_retries") > r0
        got.update(_run(engine, srcs, ("topk_bound", "balanced", "query", "power")))
        _same(got, base, "d")
        engine.reset_options()

        # e: another graph and back
        _load(engine, tiny_dangling)
        assert engine.get_batch() == 0
        engine.topk(pick_sources(tiny_dangling, 2, 413), K, epsilon=0.5)
        assert engine.get_batch() == 2
        _load(engine, g)
        assert engine.get_batch() == 0
        _same(_run(engine, srcs, CALLS), base, "e")
    finally:
        engine.set_batch(0)
        engine.reset_options()
        engine.set_balanced(False)
