"""BiPPR on the GPU (fora_hip_bwdpush_batch / fora_hip_bippr_batch) against the Python twin of tests/bippr_ref.py: the
backward push bit for bit on every target, both tiers and any chunking; the estimate bit for bit from the walks'
endpoints (fora_hip_walks); the error bound against power iteration at ws size."""
import math

import numpy as np
import pytest

import bippr_ref as br
from conftest import pick_sources

pytestmark = pytest.mark.gpu
SEED = 0x464F5241
ALPHA = 0.2
EPS = 0.5


def _load(engine, g, eps=EPS):
    engine.clear_index()
    engine.reset_options()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(alpha=ALPHA, epsilon=eps, seed=SEED)
    return engine.get_params()


_TWIN = {}


def _twin_all(g, rmax):
    key = (id(g), rmax)
    if key not in _TWIN:
        rsv = np.zeros((g.n, g.n), dtype=np.uint64)
        res = np.zeros((g.n, g.n), dtype=np.uint64)
        pops = relax = entries = levels = 0
        pushes = []
        for t in range(g.n):
            p, r, po, re, lv = br.twin_bwd_push_sparse(g, t, rmax, ALPHA)
            pushes.append((p, r))
            for v, x in p.items():
                rsv[t, v] = x
            for v, x in r.items():
                res[t, v] = x
            pops, relax, entries, levels = pops + po, relax + re, entries + br.entries_of(p, r), max(levels, lv)
        _TWIN[key] = dict(reserve=rsv, residue=res, pops=pops, relax=relax, entries=entries, levels=levels, pushes=pushes)
    return _TWIN[key]


def _ends(engine, s, W):
    return engine.walks(int(s), 0, np.full(W, s, dtype=np.int32), np.arange(W, dtype=np.uint64)).astype(np.int64)


@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling"])
def test_bwdpush_bit_exact_all_targets(engine, request, gname):
    g = request.getfixturevalue(gname)
    _load(engine, g)
    rmax = br.bippr_setting(g.n, g.m, EPS)[0]
    tw = _twin_all(g, rmax)
    targets = np.arange(g.n, dtype=np.int32)
    seen_global = []
    for opts in ({}, {"bwd_lds_cap": 0}, {"bwd_lds_cap": 40}, {"bwd_chunk": 7}):
        engine.reset_options()
        for k, v in opts.items():
            engine.set_option(k, v)
        rsv, res, bwd = engine.bwdpush(targets, rmax)
        assert (rsv == tw["reserve"]).all() and (res == tw["residue"]).all(), opts
        assert (bwd["targets"], bwd["pops"], bwd["relax"], bwd["entries"], bwd["levels"]) == \
            (g.n, tw["pops"], tw["relax"], tw["entries"], tw["levels"]), (opts, bwd)
        seen_global.append(bwd["global_targets"])
        if opts.get("bwd_chunk"):
            assert bwd["chunks"] == (g.n + 6) // 7
    engine.reset_options()
    assert seen_global[1] == g.n and 0 < seen_global[2] < g.n  # cap 0: all global; cap 40: both tiers


def test_bwdpush_hub_target_goes_global(engine, oracle):
    """Node 0 has 2000 in-edges (> the default LDS cap of 1024 entries): its push spills to the global tier."""
    n = 2100
    src = np.concatenate([np.arange(1, 2001), np.arange(n)])
    dst = np.concatenate([np.zeros(2000, dtype=np.int64), (np.arange(n) + 1) % n])
    g = oracle.Graph.from_edges(n, src.size, src, dst)
    _load(engine, g)
    rmax = 1e-4
    targets = np.array([0, 5, 2050], dtype=np.int32)
    rsv, res, bwd = engine.bwdpush(targets, rmax)
    assert bwd["global_targets"] >= 1
    pops = relax = 0
    for i, t in enumerate(targets):
        tw = br.twin_bwd_push(g, int(t), rmax, ALPHA)
        assert (rsv[i] == tw["reserve"]).all() and (res[i] == tw["residue"]).all()
        pops, relax = pops + tw["pops"], relax + tw["relax"]
    assert (bwd["pops"], bwd["relax"]) == (pops, relax)


@pytest.mark.parametrize("batch", [1, 0])
@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling"])
def test_bippr_bit_exact_vs_twin(engine, request, gname, batch):
    g = request.getfixturevalue(gname)
    params = _load(engine, g)
    rmax, omega, W = br.bippr_setting(g.n, g.m, EPS)
    live = pick_sources(g, 2, 401)
    dang = pick_sources(g, 1, 402, want_dangling=True)
    srcs = np.concatenate([dang, live, live[:1]]).astype(np.int32)  # a dangling source (where there is one) and a duplicate
    engine.set_batch(batch)
    try:
        _, fix, _, _, st, bwd = engine.bippr(srcs, epsilon=EPS)
    finally:
        engine.set_batch(0)
    assert engine.get_params() == params
    tw = _twin_all(g, rmax)
    assert (bwd["targets"], bwd["pops"], bwd["relax"], bwd["entries"]) == (g.n, tw["pops"], tw["relax"], tw["entries"])
    for i, s in enumerate(srcs):
        assert st[i]["n_walks"] == W and st[i]["rmax_used"] == rmax
        assert st[i]["pops"] == 0 and st[i]["n_rw"] == 0
        want = br.twin_bippr(g, int(s), rmax, W, _ends(engine, s, W), ALPHA, pushes=tw["pushes"])
        assert (fix[i] == want).all(), (i, s)
        assert st[i]["ppr_sum_fix"] == int(want.sum(dtype=np.uint64))
    assert (fix[-1] == fix[len(dang)]).all()


def test_bippr_dangling_source(engine, tiny_dangling):
    g = tiny_dangling
    _load(engine, g)
    s = int(pick_sources(g, 1, 411, want_dangling=True)[0])
    ppr, fix, _, _, st, _ = engine.bippr([s], epsilon=EPS, want_ppr=True)
    keep = (br.BWD_ONE * int(math.ldexp(ALPHA, 62))) >> 62
    want = np.zeros(g.n, dtype=np.uint64)
    want[s] = keep
    assert st[0]["dangling_source"] == 1 and (fix[0] == want).all()
    assert ppr[0][s] == math.ldexp(keep, -60) and np.count_nonzero(ppr[0]) == 1


def test_bippr_rmax_over_one_is_monte_carlo_over_four(engine, tiny):
    g = tiny
    _load(engine, g)
    rmax, _, W = br.bippr_setting(g.n, g.m, EPS, rmax_scale=4.0)
    assert 1.0 <= rmax < 3.0 * ALPHA * 5
    srcs = pick_sources(g, 2, 421)
    _, fix, _, _, st, bwd = engine.bippr(srcs, epsilon=EPS, rmax_scale=4.0)
    assert bwd["pops"] == 0 and bwd["relax"] == 0 and bwd["entries"] == g.n
    for i, s in enumerate(srcs):
        assert st[i]["n_walks"] == W and st[i]["rmax_used"] == rmax
        assert (fix[i] == br.mc_slab(g.n, _ends(engine, s, W)) // np.uint64(4)).all()


def test_bippr_topk_matches_dense_output(engine, tiny_dangling):
    g = tiny_dangling
    _load(engine, g)
    srcs = np.concatenate([pick_sources(g, 2, 431), pick_sources(g, 1, 432, want_dangling=True)]).astype(np.int32)
    k = 50
    _, fix, ids, sc, _, _ = engine.bippr(srcs, epsilon=EPS, k=k)
    for i in range(srcs.size):
        nz = np.flatnonzero(fix[i])
        order = sorted(nz.tolist(), key=lambda v: (-int(fix[i][v]), v))[:k]
        want_ids = np.zeros(k, dtype=np.int32)
        want_sc = np.zeros(k)
        want_ids[:len(order)] = order
        want_sc[:len(order)] = [math.ldexp(int(fix[i][v]), -60) for v in order]
        assert (ids[i] == want_ids).all() and (sc[i] == want_sc).all(), i
    assert (sc[-1][1:] == 0).all() and (ids[-1][1:] == 0).all()  # the dangling source: one entry, then the padding


def test_bippr_webstanford_error_bound(engine):
    from fora_amd import synth
    n, m, rp, col = synth.preset("webstanford")
    engine.clear_index()
    engine.reset_options()
    engine.set_graph(n, m, rp, col)
    engine.set_params(alpha=ALPHA, epsilon=EPS, seed=SEED)
    rmax, omega, W = br.bippr_setting(n, m, EPS)
    srcs = synth.query_set(n, 2, 7)
    ppr, _, _, _, st, bwd = engine.bippr(srcs, epsilon=EPS, want_ppr=True, want_fix=False)
    assert m <= bwd["entries"] <= 3 * m and bwd["targets"] == n
    assert bwd["bwd_ms"] > 0 and bwd["walk_ms"] > 0 and bwd["combine_ms"] > 0
    exact, _, _, _ = engine.power_iteration(srcs)
    for i in range(srcs.size):
        assert st[i]["n_walks"] == W
        big = exact[i] >= 1.0 / n
        bad = np.abs(ppr[i] - exact[i])[big] > EPS * exact[i][big]
        assert bad.sum() <= 1, (i, int(bad.sum()))


def test_fora_not_disturbed_and_argument_errors(engine, oracle, small):
    from fora_amd import ForaError
    g = small
    params = _load(engine, g)
    srcs = pick_sources(g, 4, 441)
    a_ppr, a_res, _ = engine.query_fix(srcs)
    B = engine.get_batch()
    engine.bippr(srcs[:2], epsilon=EPS, k=5)
    engine.bwdpush(srcs, 0.05)
    assert engine.get_params() == params and engine.get_batch() == B
    b_ppr, b_res, _ = engine.query_fix(srcs)
    assert (a_ppr == b_ppr).all() and (a_res == b_res).all()
    good = np.array([1, 2], dtype=np.int32)
    bad_calls = [
        lambda: engine.bippr(np.array([g.n], dtype=np.int32)),
        lambda: engine.bippr(np.array([-1], dtype=np.int32)),
        lambda: engine.bippr(good, epsilon=0.0),
        lambda: engine.bippr(good, rmax_scale=0.0),
        lambda: engine.bippr(good, k=2000),
        lambda: engine.bippr(good, rmax_scale=1e6),  # rmax / alpha beyond the 2^60 fixed point
        lambda: engine.bwdpush(np.array([g.n], dtype=np.int32), 0.1),
        lambda: engine.bwdpush(good, 0.0),
        lambda: engine.bwdpush(good, 15 * ALPHA),  # 1 + rmax / alpha == 16
    ]
    for call in bad_calls:
        with pytest.raises(ForaError) as e:
            call()
        assert e.value.code == -1
    assert engine.get_params() == params and engine.get_batch() == B
    c_ppr, _, _ = engine.query_fix(srcs)
    assert (a_ppr == c_ppr).all()
