"""Top-k sparse rows of seed sets on the GPU (fora_hip_seeds_sparse_topk_batch, Engine.query_seeds_sparse_topk): the set rows
cut to their k largest entries AFTER the sum.  The expected rows never pass through the new code: they are the dense set rows
of Engine.query_seeds (pinned to tests/seeds_ref.py by test_seeds_gpu.py) through the numpy twin tests/sparse_topk_ref.py.
Every comparison is an equality."""
import numpy as np
import pytest

import seeds_outputs_ref as so
from fora_amd import synth
from sparse_topk_ref import check_topk

pytestmark = pytest.mark.gpu
KS = (1, 7, 64, 10 ** 9)


@pytest.fixture(scope="module")
def odd(oracle):
    """n odd: every other row of the accumulator block starts at an odd word (no 16-byte alignment)."""
    src, dst = synth.rmat_graph(1999, 16000, 20260118)
    return oracle.Graph.from_edges(1999, 16000, src, dst)


def _dense(engine, sets, weights):
    r = engine.query_seeds(sets, weights=weights, want_fix=True)
    return r["fix"], r["row_sum_fix"]


def _check(engine, g, sets, weights, rows, sums, k, t=None, **kw):
    thr = so.thr_fix_of(1.0 / g.n if t is None else t)
    out = engine.query_seeds_sparse_topk(sets, k, weights=weights, threshold=t, want_fix=True, **kw)
    lens = check_topk(rows, thr, k, out["row_ptr"], out["ids"], out["fix"], out["sparse"], out["topk"])
    assert np.array_equal(out["vals"], np.ldexp(out["fix"].astype(np.float64), -62))
    assert (out["row_sum_fix"] == sums).all()                       # over the WHOLE row, not over the kept part
    assert out["topk"]["chunks"] >= 1 and out["topk"]["select_ms"] >= 0
    return out, lens


@pytest.mark.parametrize("gname", ["tiny_dangling", "odd"])
def test_set_rows_equal_the_twin(engine, request, gname):
    """uniform and weighted sets, a set of dangling seeds, duplicate sets (seeds_outputs_ref.sets_of)"""
    g = request.getfixturevalue(gname)
    so.load(engine, g)
    sets, weights = so.sets_of(g)
    for w in (None, weights):
        rows, sums = _dense(engine, sets, w)
        cut = 0
        for t in (None, 0.0):
            for k in KS:
                out, lens = _check(engine, g, sets, w, rows, sums, k, t)
                cut += out["topk"]["cut_rows"]
                if k == 10 ** 9:
                    plain = engine.query_seeds_sparse(sets, weights=w, threshold=t, want_fix=True)
                    for name in ("row_ptr", "ids", "vals", "fix"):
                        assert (out[name] == plain[name]).all(), name
        assert cut > 0
        if gname == "tiny_dangling":   # the set of dangling seeds only: at most two entries, whatever k
            assert (rows[3] != 0).sum() <= 2


def test_a_uniform_singleton_equals_query_sparse_topk(engine, tiny_dangling):
    g = tiny_dangling
    so.load(engine, g)
    seeds = so.pick(g, 3, 611) + so.pick(g, 1, 612, want_dangling=True)
    for k in (1, 7, 64):
        for t in (None, 0.0):
            row_ptr, ids, vals, fix, st, sp, tk = engine.query_sparse_topk(np.array(seeds, np.int32), k, threshold=t, want_fix=True)
            out = engine.query_seeds_sparse_topk([[s] for s in seeds], k, threshold=t, want_fix=True)
            assert (out["row_ptr"] == row_ptr).all() and (out["ids"] == ids).all() and (out["fix"] == fix).all()
            assert out["topk"]["cut_rows"] == tk["cut_rows"] and (k > 1 or tk["cut_rows"] == 3)
    lo = int(row_ptr[3])
    assert row_ptr[4] - lo == 1 and ids[lo] == seeds[3] and fix[lo] == so.ONE    # the dangling seed: (s, 2^62) for every k


@pytest.mark.parametrize("gname", ["tiny_dangling", "odd"])
@pytest.mark.parametrize("config", [dict(seeds_rows=1), dict(seeds_rows=2), dict(seeds_dedup=0), dict(batch=4),
                                    dict(seeds_rows=1, topk_cand=1, topk_lds_cap=0), dict(seeds_rows=3, topk_cand=1, topk_lds_cap=64)],
                         ids=lambda c: "_".join(f"{k}{v}" for k, v in c.items()))
def test_same_bits_whatever_the_chunking_dedup_and_tier(engine, request, gname, config):
    g = request.getfixturevalue(gname)
    so.load(engine, g)
    sets, weights = so.sets_of(g)
    rows, sums = _dense(engine, sets, weights)
    kw = dict(config)
    batch = kw.pop("batch", 0)
    try:
        for name, v in kw.items():
            engine.set_option(name, v)
        engine.set_batch(batch)
        for k in (7, 64):
            out, lens = _check(engine, g, sets, weights, rows, sums, k, 0.0)
            tk = out["topk"]
            assert tk["cut_rows"] > 0
            if "seeds_rows" in kw:
                chunk = kw["seeds_rows"] + (kw["seeds_rows"] & g.n & 1)   # an odd n: rounded up to even
                assert out["sparse"]["batches"] == -(-len(sets) // chunk)
                assert tk["chunks"] >= out["sparse"]["batches"] > 1
            if kw.get("topk_lds_cap") == 0:
                assert tk["global_rows"] == tk["cut_rows"] and tk["lds_rows"] == 0
            if kw.get("topk_lds_cap") == 64:
                assert tk["global_rows"] == int((lens > 64).sum()) and tk["lds_rows"] == int(((lens > k) & (lens <= 64)).sum())
            if "topk_lds_cap" not in kw:
                assert tk["lds_rows"] == tk["cut_rows"]
    finally:
        engine.reset_options()
        engine.set_batch(0)
