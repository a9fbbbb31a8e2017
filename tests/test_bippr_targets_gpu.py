"""Targeted BiPPR on the GPU (fora_hip_bippr_targets_batch, Engine.bippr_targets): pi(s, t) for chosen sources and
targets.  Every word is checked against two values that do not pass through the new code: (a) the columns of
Engine.bippr, the single-source form with its n pushes, and (b) the estimate formula written out below, over the Python
twin's pushes of the listed targets only (tests/bippr_ref.py) and the walk slab of the walks' endpoints
(fora_hip_walks)."""
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
    engine.set_batch(0)
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(alpha=ALPHA, epsilon=eps, seed=SEED)
    return engine.get_params()


_PUSH = {}


def _push(g, t, rmax):
    """(reserve dict, residue dict, pops, relax, levels, entries) of the twin's push to t, once per (graph, rmax, t)."""
    key = (id(g), rmax, int(t))
    if key not in _PUSH:
        p, r, pops, relax, levels = br.twin_bwd_push_sparse(g, int(t), rmax, ALPHA)
        _PUSH[key] = (g, p, [(v, x) for v, x in r.items() if x], pops, relax, levels, br.entries_of(p, r))
    return _PUSH[key][1:]


def _slab(engine, g, s, W):
    """Walk slab of source s at 2^-62 as Python ints, from the endpoints of its W walks."""
    ends = engine.walks(int(s), 0, np.full(W, s, dtype=np.int32), np.arange(W, dtype=np.uint64)).astype(np.int64)
    return br.mc_slab(g.n, ends).tolist()


def _expect(engine, g, srcs, targets, rmax, W):
    """(b): est[i][j] = p_t[s] + sum_v floor(c_s[v] * r_t[v] / 2^62), every term floored on its own; and the counters'
    sums over the listed targets, duplicates counted each time."""
    slabs = {}
    out = np.zeros((len(srcs), len(targets)), dtype=np.uint64)
    for i, s in enumerate(int(x) for x in srcs):
        if s not in slabs:
            slabs[s] = _slab(engine, g, s, W)
        c = slabs[s]
        for j, t in enumerate(int(x) for x in targets):
            p, r = _push(g, t, rmax)[:2]
            acc = p.get(s, 0) + sum((c[v] * x) >> 62 for v, x in r if c[v])
            assert acc <= br.U64
            out[i, j] = acc
    tot = [sum(_push(g, int(t), rmax)[k] for t in targets) for k in (2, 3, 5)]
    levels = max(_push(g, int(t), rmax)[4] for t in targets)
    return out, dict(pops=tot[0], relax=tot[1], entries=tot[2], levels=levels)


def _sources(g):
    live = pick_sources(g, 2, 501)
    dang = pick_sources(g, 1, 502, want_dangling=True)
    return np.concatenate([dang, live, live[:1]]).astype(np.int32)  # a dangling one where there is one, and a duplicate


def _targets(g, srcs, seed=503, count=40):
    """About `count` targets, shuffled, with duplicates: every source, a dangling node (where there is one), a node
    without in-edges and the node of largest in-degree among them."""
    indeg = np.bincount(g.col[:int(g.row_ptr[-1])], minlength=g.n)
    rng = np.random.Generator(np.random.PCG64(seed))
    must = list(np.unique(srcs)) + [int(np.flatnonzero(indeg == 0)[0]), int(indeg.argmax())]
    must += [int(x) for x in np.flatnonzero(g.deg == 0)[:1]]
    rest = rng.choice(g.n, count - len(must) - 3, replace=False).tolist()
    tg = np.array(must + rest + rest[:2] + [int(indeg.argmax())], dtype=np.int32)
    rng.shuffle(tg)
    return tg


def _check_stats(st, srcs, g, fix, W, rmax):
    for i, s in enumerate(srcs):
        assert st[i]["n_walks"] == W and st[i]["rmax_used"] == rmax
        assert st[i]["dangling_source"] == int(g.deg[s] == 0)
        assert st[i]["ppr_sum_fix"] == int(fix[i].sum(dtype=np.uint64))
        for f in ("rsum", "rsum_fix", "n_rw", "n_idx_hit", "pops", "relax", "levels", "push_rounds"):
            assert st[i][f] == 0, f


@pytest.mark.parametrize("batch", [1, 0])
@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling"])
def test_columns_of_bippr_and_the_formula(engine, request, gname, batch):
    g = request.getfixturevalue(gname)
    params = _load(engine, g)
    rmax, _, W = br.bippr_setting(g.n, g.m, EPS)
    srcs = _sources(g)
    tg = _targets(g, srcs)
    assert len(set(tg.tolist())) < tg.size and set(srcs.tolist()) <= set(tg.tolist())
    engine.set_batch(batch)
    try:
        est, fix, st, bwd = engine.bippr_targets(srcs, tg, epsilon=EPS, want_est=True)
        _, full, _, _, _, _ = engine.bippr(srcs, epsilon=EPS)
    finally:
        engine.set_batch(0)
    assert engine.get_params() == params
    assert fix.shape == (srcs.size, tg.size) and est.shape == fix.shape
    assert (fix == full[:, tg]).all()                                   # (a)
    want, cnt = _expect(engine, g, srcs, tg, rmax, W)
    assert (fix == want).all()                                          # (b)
    assert (est == np.ldexp(fix.astype(np.float64), -60)).all()
    assert all(math.ldexp(int(fix[i, j]), -60) == est[i, j] for i in range(srcs.size) for j in range(0, tg.size, 7))
    _check_stats(st, srcs, g, fix, W, rmax)
    assert (bwd["targets"], bwd["pops"], bwd["relax"], bwd["entries"], bwd["levels"]) == \
        (tg.size, cnt["pops"], cnt["relax"], cnt["entries"], cnt["levels"])
    assert bwd["chunks"] == 1
    if g.deg[srcs[0]] == 0:  # the dangling source: keep(2^60) where the target is the source, 0 elsewhere
        keep = (br.BWD_ONE * int(math.ldexp(ALPHA, 62))) >> 62
        assert (fix[0] == np.where(tg == srcs[0], np.uint64(keep), np.uint64(0))).all()
    assert (fix[-1] == fix[-3]).all()  # the duplicate source


def test_all_targets_is_the_single_source_form(engine, tiny_dangling):
    g = tiny_dangling
    _load(engine, g)
    srcs = _sources(g)
    _, full, _, _, st_full, bwd_full = engine.bippr(srcs, epsilon=EPS)
    _, fix, st, bwd = engine.bippr_targets(srcs, np.arange(g.n, dtype=np.int32), epsilon=EPS)
    assert (fix == full).all()
    assert (st["ppr_sum_fix"] == st_full["ppr_sum_fix"]).all() and (st["n_walks"] == st_full["n_walks"]).all()
    for f in ("targets", "pops", "relax", "entries", "global_targets", "levels", "chunks"):
        assert bwd[f] == bwd_full[f], f


def test_options_change_no_bit(engine, tiny_dangling):
    """rmax_scale 0.05: rmax 0.01418, W 2822, up to 600 - 750 entries per target.  Tier, chunking, batching, lane mapping
    and span: the same bits."""
    g = tiny_dangling
    _load(engine, g)
    rmax, _, W = br.bippr_setting(g.n, g.m, EPS, rmax_scale=0.05)
    assert W == 2822
    srcs = _sources(g)
    tg = _targets(g, srcs, seed=511)
    want, cnt = _expect(engine, g, srcs, tg, rmax, W)
    runs = [({}, 0), ({"bwd_lds_cap": 0}, 0), ({"bwd_lds_cap": 40}, 0), ({"bwd_chunk": 7}, 2),
            ({"tgt_lanes": 0}, 0), ({"tgt_lanes": 1}, 0), ({"tgt_lanes": 0, "tgt_span": 100, "bwd_chunk": 7}, 3),
            ({"tgt_lanes": 1, "tgt_span": 1000}, 0), ({"tgt_span": 1}, 0)]
    try:
        for opts, batch in runs:
            engine.reset_options()
            for k, v in opts.items():
                engine.set_option(k, v)
            engine.set_batch(batch)
            _, fix, st, bwd = engine.bippr_targets(srcs, tg, epsilon=EPS, rmax_scale=0.05)
            assert (fix == want).all(), opts
            _check_stats(st, srcs, g, fix, W, rmax)
            assert (bwd["targets"], bwd["pops"], bwd["relax"], bwd["entries"], bwd["levels"]) == \
                (tg.size, cnt["pops"], cnt["relax"], cnt["entries"], cnt["levels"]), opts
            if "bwd_chunk" in opts:
                assert bwd["chunks"] == (tg.size + 6) // 7
                assert srcs.size > batch  # at least two source batches: every batch writes the chunks again
            else:
                assert bwd["chunks"] == 1
            if opts.get("bwd_lds_cap") == 0:
                assert bwd["global_targets"] == tg.size
            if opts.get("bwd_lds_cap") == 40:
                assert 0 < bwd["global_targets"] < tg.size  # both tiers
    finally:
        engine.reset_options()
        engine.set_batch(0)


@pytest.fixture(scope="module")
def hub(oracle):
    """2000 nodes pointing at node 0, plus a ring: the graph of test_bwdpush_hub_target_goes_global."""
    n = 2100
    src = np.concatenate([np.arange(1, 2001), np.arange(n)])
    dst = np.concatenate([np.zeros(2000, dtype=np.int64), (np.arange(n) + 1) % n])
    return oracle.Graph.from_edges(n, src.size, src, dst)


@pytest.mark.parametrize("nsrc", [1, 3, 64, 65])
def test_one_heavy_target_across_the_wave_width(engine, hub, nsrc):
    """Target 0 at rmax_scale 0.1 (rmax 0.013965, W 2936): 4032 non-zero reserve / residue words on 2021 entry rows, on
    the global tier.  Written for spans of S = 64 entry rows per wave, the span the library picks for chunks this small (32
    spans over target 0), and for the forced spans 100 (21 spans, no multiple of the 64-entry tile) and 1000 (3 spans).
    1 and 3 sources run lane = entry, 64 and 65 lane = slot, in one batch each; both mappings are also forced at every
    width."""
    g = hub
    _load(engine, g)
    rmax, _, W = br.bippr_setting(g.n, g.m, EPS, rmax_scale=0.1)
    assert W == 2936
    ids = np.array([7, 0, 1500, 2050, 5], dtype=np.int32)
    srcs = ids[np.arange(nsrc) % ids.size]
    try:
        for tg in (np.array([0], dtype=np.int32), np.array([0, 5, 2050, 0], dtype=np.int32)):
            want, cnt = _expect(engine, g, srcs, tg, rmax, W)
            assert _push(g, 0, rmax)[5] >= 4032
            for opts in ({}, {"tgt_lanes": 0}, {"tgt_lanes": 1}, {"tgt_span": 100}, {"tgt_lanes": 0, "tgt_span": 1000},
                         {"tgt_lanes": 1, "tgt_span": 1000}):
                engine.reset_options()
                for k, v in opts.items():
                    engine.set_option(k, v)
                _, fix, st, bwd = engine.bippr_targets(srcs, tg, epsilon=EPS, rmax_scale=0.1)
                assert engine.get_batch() >= nsrc  # one batch
                assert bwd["global_targets"] >= 1 and bwd["entries"] >= 4032
                assert (bwd["pops"], bwd["relax"], bwd["entries"]) == (cnt["pops"], cnt["relax"], cnt["entries"])
                assert (fix == want).all(), (opts, tg)
                _check_stats(st, srcs, g, fix, W, rmax)
    finally:
        engine.reset_options()


def test_edges_of_the_argument_space(engine, tiny_dangling):
    from fora_amd import ForaError
    g = tiny_dangling
    params = _load(engine, g)
    rmax, _, W = br.bippr_setting(g.n, g.m, EPS)
    srcs = _sources(g)
    _, full, _, _, _, _ = engine.bippr(srcs, epsilon=EPS)
    none = np.zeros(0, dtype=np.int32)

    # no targets: the sources' stats, nothing else; no sources: nothing
    est, fix, st, bwd = engine.bippr_targets(srcs, none, want_est=True)
    assert fix.shape == (srcs.size, 0) and est.shape == (srcs.size, 0)
    _check_stats(st, srcs, g, fix, W, rmax)
    assert all(v == 0 for v in bwd.values())
    est, fix, st, bwd = engine.bippr_targets(none, np.array([1, 2], dtype=np.int32), want_est=True)
    assert fix.shape == (0, 2) and len(st) == 0 and all(v == 0 for v in bwd.values())

    # one target; every node twice and three more
    t = int(srcs[1])
    _, fix, st, bwd = engine.bippr_targets(srcs, [t])
    assert (fix[:, 0] == full[:, t]).all() and bwd["targets"] == 1
    _check_stats(st, srcs, g, fix, W, rmax)
    tg = np.concatenate([np.arange(g.n), np.arange(g.n)[::-1], [5, 0, g.n - 1]]).astype(np.int32)
    assert tg.size == 2 * g.n + 3
    _, fix, st, bwd = engine.bippr_targets(srcs, tg)
    assert (fix == full[:, tg]).all() and bwd["targets"] == tg.size
    _check_stats(st, srcs, g, fix, W, rmax)

    good = np.array([1, 2], dtype=np.int32)
    bad_calls = [
        lambda: engine.bippr_targets(good, np.array([3, -1], dtype=np.int32)),
        lambda: engine.bippr_targets(good, np.array([g.n, 3], dtype=np.int32)),
        lambda: engine.bippr_targets(np.array([g.n], dtype=np.int32), good),
        lambda: engine.bippr_targets(np.array([-1], dtype=np.int32), good),
        lambda: engine.bippr_targets(good, good, epsilon=0.0),
        lambda: engine.bippr_targets(good, good, rmax_scale=0.0),
        lambda: engine.bippr_targets(good, good, rmax_scale=float("nan")),
        lambda: engine.bippr_targets(good, good, rmax_scale=float("inf")),
        lambda: engine.bippr_targets(good, good, rmax_scale=16 * ALPHA / rmax),  # 1 + rmax / alpha >= 16
    ]
    assert 1 + br.bippr_setting(g.n, g.m, EPS, rmax_scale=16 * ALPHA / rmax)[0] / ALPHA >= 16
    for k, call in enumerate(bad_calls):
        with pytest.raises(ForaError) as e:
            call()
        assert e.value.code == -1, k
        _, fix, _, _ = engine.bippr_targets(srcs[:2], [t])  # the engine still answers
        assert (fix[:, 0] == full[:2, t]).all(), k
    assert engine.get_params() == params

    # rmax >= 1: nothing pops, every word is the walk slab's over four
    r4, _, W4 = br.bippr_setting(g.n, g.m, EPS, rmax_scale=4.0)
    assert 1.0 <= r4 and 1 + max(1.0, r4 / ALPHA) < 16
    tg = _targets(g, srcs, seed=521)
    _, fix, st, bwd = engine.bippr_targets(srcs, tg, rmax_scale=4.0)
    assert bwd["pops"] == 0 and bwd["relax"] == 0 and bwd["entries"] == tg.size
    for i, s in enumerate(srcs):
        c = np.array(_slab(engine, g, s, W4), dtype=np.uint64)
        assert (fix[i] == c[tg] >> np.uint64(2)).all()
        assert st[i]["n_walks"] == W4 and st[i]["rmax_used"] == r4


def test_nothing_else_disturbed(engine, small):
    g = small
    params = _load(engine, g)
    srcs = pick_sources(g, 4, 531)
    a_ppr, a_res, _ = engine.query_fix(srcs)
    B = engine.get_batch()
    sizes = engine.index_sizes()
    row_ptr, ids, vals, fx, _, _ = engine.query_sparse(srcs, want_fix=True)
    tg = pick_sources(g, 30, 532)
    engine.bippr_targets(srcs[:3], tg, epsilon=EPS, want_est=True)
    ids2, vals2, fx2 = np.zeros_like(ids), np.zeros_like(vals), np.zeros_like(fx)
    engine.sparse_fetch(ids2, vals2, fx2, cap=ids.size)  # the held sparse result, again
    assert (ids2 == ids).all() and (vals2 == vals).all() and (fx2 == fx).all()
    assert engine.get_params() == params and engine.get_batch() == B
    after = engine.index_sizes()
    assert after[0] == sizes[0] and (after[1] == sizes[1]).all() and (after[2] == sizes[2]).all()
    b_ppr, b_res, _ = engine.query_fix(srcs)
    assert (a_ppr == b_ppr).all() and (a_res == b_res).all()
    engine.sparse_clear()
