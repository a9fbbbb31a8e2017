"""Accounting of fora_timing (fora_hip.hip: the event pairs around the launches, ev_collect, fold_counters): a call adds
its own launches and counters and nothing else -- the same call twice counts twice, the attempts a bucket retry threw
away count nothing, and with the `profile` option off only the event-borne fields stay zero."""
import numpy as np
import pytest

from conftest import pick_sources

pytestmark = pytest.mark.gpu
SEED = 0x464F5241
K = 8
MS = ("push_pop_ms", "push_expand_ms", "push_accum_ms", "walk_alloc_ms", "walk_ms", "walk_accum_ms", "other_ms", "batch_ms",
      "push_tail_ms", "push_team_ms")
LAUNCHES = ("push_pop_launches", "push_expand_launches", "push_accum_launches", "walk_launches", "push_tail_launches",
            "push_team_launches")
INTS = LAUNCHES + ("levels", "batches", "pops", "relax", "walks", "idx_hits", "walk_steps")


def _sources(g):
    live, dang = pick_sources(g, 6, 411), pick_sources(g, 1, 412, want_dangling=True)
    srcs = np.concatenate([live[:2], dang, live[2:]]).astype(np.int32)
    assert srcs.size == 7 and (g.deg[srcs] == 0).sum() == 1
    return srcs


def _load(engine, g):
    engine.reset_options()
    engine.set_batch(0)
    engine.set_balanced(False)
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(epsilon=0.5, seed=SEED)


def _timed(engine, call, times=1):
    """fora_timing of `times` runs of call() from a reset, and the last run's result arrays as bytes."""
    engine.reset_timing()
    for _ in range(times):
        out = call()
    t = engine.timing()
    assert set(MS) | set(INTS) == set(t), "a fora_timing field this test does not know"
    print({k: t[k] for k in INTS}, {k: round(t[k], 3) for k in MS})
    return t, tuple(np.ascontiguousarray(a).tobytes() for a in out)


@pytest.fixture(scope="module")
def query_once(engine, small_dangling):
    """(sources, timing, result bytes) of one profiled query_fix on a planned workspace."""
    _load(engine, small_dangling)
    srcs = _sources(small_dangling)
    engine.query_fix(srcs)
    t1, out = _timed(engine, lambda: engine.query_fix(srcs)[:2])
    return srcs, t1, out


def _additive(engine, call, t1):
    t2, _ = _timed(engine, call, times=2)
    for k in INTS:
        assert t2[k] == 2 * t1[k], k
    for t in (t1, t2):
        assert t["batch_ms"] > 0 and t["walk_ms"] > 0
        assert t["push_pop_ms"] == 0  # the bucketed layout never launches k_push_pop


def test_same_call_twice_counts_twice(engine, query_once):
    srcs, t1, _ = query_once
    _additive(engine, lambda: engine.query_fix(srcs)[:2], t1)
    topk = lambda: engine.topk(srcs, K, epsilon=0.5)
    topk()
    _additive(engine, topk, _timed(engine, topk)[0])


def test_retried_call_leaves_no_trace(engine, small_dangling, query_once):
    srcs = query_once[0]
    topk = lambda: engine.topk(srcs, K, epsilon=0.5)
    try:
        _load(engine, small_dangling)
        engine.set_option("bkcap", 8)  # buckets and overflow list far too small: leg d of test_workspace_lifecycle_gpu
        engine.set_option("ovcap", 64)
        engine.set_option("tail", 0)
        r0 = engine.get_option("bucket_retries")
        ta, out_a = _timed(engine, topk)
        r1 = engine.get_option("bucket_retries")
        tb, out_b = _timed(engine, topk)
        assert r1 > r0
        assert engine.get_option("bucket_retries") == r1
        for k in INTS:  # the forgotten attempts added nothing; the surviving one ran on the plan the second call reuses
            assert ta[k] == tb[k], k
        assert out_a == out_b
    finally:
        engine.reset_options()


def test_profile_off_keeps_the_counters(engine, small_dangling, query_once):
    srcs, t1, out1 = query_once
    try:
        _load(engine, small_dangling)
        engine.set_option("profile", 0)
        t0, out0 = _timed(engine, lambda: engine.query_fix(srcs)[:2])
        for k in MS + LAUNCHES:
            assert t0[k] == 0, k
        for k in ("pops", "relax", "walks", "levels"):  # (`batches` is counted from the batch's event pair: 0 here, like batch_ms)
            assert t0[k] == t1[k], k
        assert out0 == out1
    finally:
        engine.reset_options()
