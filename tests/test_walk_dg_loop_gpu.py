"""The main loop of k_walk_dg (online walks over the degree-grouped copy) against the twin, bit for bit, on the paths a
default query hardly takes: walks of more than 512 / 1024 steps (the rare branch that moves Philox counter word 3 on),
tiles replaced while their walks still run (tag / gen / self sums), out-degree 0 (classes and hub records), weights
that do not fit the packed stage word, full result buckets, the variant with one gather per walk, other hub counts, and
an indexed query in which k_walk_idx fills the same buckets through the shared stage first.

Weights: a walk of node v carries residue[v] / count[v] (+1), about 2^62 / omega.  From omega = 2^18 down every weight is
at least WPACK_MAXW = 2^44 and leaves by a direct atomic instead of the wave's stage; the cases that are about the stage
therefore set rmax and omega directly (omega > 2^18, and a small rmax where few walks per item are wanted)."""
import numpy as np
import pytest

from conftest import pick_sources

pytestmark = pytest.mark.gpu
SEED = 0x464F5241
LONG_ALPHA = 0.004            # mean walk length 250 steps: 13 % of the walks pass 512 steps, 1.6 % pass 1024
WPACK_MAXW = 1 << 44          # fora_kernels.h: weight bits of a staged result
FEW_RMAX, FEW_OMEGA = 4e-7, 300000.0   # tiny: ~960 items of mostly 1-2 walks each, every weight below 2^44 (rsum ~ 0.003)


def _load_raw(engine, g, alpha, rmax, omega, opt=False):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params_raw(alpha, rmax, omega, opt=opt, seed=SEED)


def _load(engine, g, opt=False, epsilon=0.5):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(epsilon=epsilon, opt=opt, seed=SEED)
    return engine.get_params()


def _same_as_twin(engine, oracle, g, srcs, rmax, omega, alpha=0.2, opt=False, index=None):
    srcs = np.asarray(srcs, dtype=np.int32)
    ppr, res, st = engine.query_fix(srcs, with_idx=index is not None)
    twins = []
    for i, s in enumerate(srcs):
        want, wres, wst = oracle.twin_query(g, int(s), rmax, omega, alpha=alpha, opt=opt, seed=SEED, index=index)
        assert (res[i] == wres).all(), ("residue", int(s))
        assert (ppr[i] == want).all(), ("ppr", int(s), int((ppr[i] != want).sum()))
        assert st[i]["n_walks"] == wst["n_walks"] and st[i]["n_idx_hit"] == wst["n_idx_hit"]
        assert st[i]["ppr_sum_fix"] == oracle.FIX_ONE                      # mass conserved exactly
        assert int(want.sum(dtype=np.uint64)) == oracle.FIX_ONE
        twins.append((want, wres, wst))
    return ppr, st, twins


def _weights(oracle, g, twin, omega, alpha=0.2, opt=False):
    """(walk count, smallest weight) of every walk item of a twin query: incr = residue / count, weights incr and incr + 1."""
    _, res, st = twin
    _, cnt = oracle.twin_walk_counts(g, res, st["rsum_fix"], omega, alpha=alpha, opt=opt)
    nz = cnt > 0
    return cnt[nz], res[nz] // cnt[nz]


def _dg_hub_set(g, dg_hubs=0):
    """The hub records of the degree-grouped copy: the H nodes of largest out-degree (ties by id), H the first of
    256 ... 4096 (not below dg_hubs) that leaves at most 255 distinct degrees behind it; every node up to 256 nodes."""
    deg = np.asarray(g.deg)
    order = np.argsort(-deg.astype(np.int64), kind="stable")
    if g.n <= 256:
        return set(order.tolist())
    for h in (256, 512, 1024, 2048, 4096):
        if dg_hubs > 0 and h < dg_hubs:
            continue
        hh = min(h, g.n)
        if len(np.unique(deg[order[hh:]])) <= 255:
            return set(order[:hh].tolist())
    raise AssertionError("the graph has no degree-grouped copy")


@pytest.fixture(scope="module")
def long_pairs(oracle, tiny):
    """~600 (start, j) pairs on `tiny` and the twin's step count and endpoint of each walk at alpha 0.004."""
    rng = np.random.Generator(np.random.PCG64(7))
    starts = rng.integers(0, tiny.n, 600).astype(np.int32)
    js = rng.integers(0, 1 << 40, 600).astype(np.uint64)
    steps = np.array([oracle.walk_steps(tiny, SEED, 5, 0, int(a), int(j), alpha=LONG_ALPHA) for a, j in zip(starts, js)])
    ends = np.array([oracle.walk(tiny, SEED, 5, 0, int(a), int(j), alpha=LONG_ALPHA) for a, j in zip(starts, js)], dtype=np.int32)
    return starts, js, steps, ends


def test_long_walks_take_the_rare_philox_branch(engine, oracle, tiny, long_pairs):
    g = tiny
    starts, js, steps, ends = long_pairs
    assert (steps > 512).sum() >= 20 and (steps > 1024).sum() >= 3, ((steps > 512).sum(), (steps > 1024).sum())
    _load_raw(engine, g, LONG_ALPHA, FEW_RMAX, FEW_OMEGA)
    assert (engine.walks(5, 0, starts, js) == ends).all()
    # a batch of 4 sources through k_walk_dg: ~1500 walks each, a sixth of them past 512 steps
    srcs = pick_sources(g, 4, 411)
    _, st, twins = _same_as_twin(engine, oracle, g, srcs, FEW_RMAX, FEW_OMEGA, alpha=LONG_ALPHA)
    for i, (_, _, wst) in enumerate(twins):
        assert wst["walk_steps"] > 150 * wst["n_walks"] > 0                # long walks indeed (mean 1 / alpha = 250)
        cnt, w = _weights(oracle, g, twins[i], FEW_OMEGA, alpha=LONG_ALPHA)
        assert int(w.max()) + 1 < WPACK_MAXW                               # ... and every result goes through the wave's stage
    tm_steps = sum(t[2]["walk_steps"] for t in twins)
    engine.reset_timing()
    engine.query_fix(srcs, want_residue=False)
    assert engine.timing()["walk_steps"] == tm_steps


def test_walks_outlive_their_tile(engine, oracle, tiny):
    """One workgroup per slot: its 8 waves share ~30 tiles of 32 items, an item has 1-2 walks, a walk runs for ~125
    iterations -- a wave replaces its tile about every iteration while earlier tiles' walks are still under way."""
    g = tiny
    engine.set_option("xb", 1)
    try:
        _load_raw(engine, g, LONG_ALPHA, FEW_RMAX, FEW_OMEGA)
        srcs = pick_sources(g, 3, 412)
        _, _, twins = _same_as_twin(engine, oracle, g, srcs, FEW_RMAX, FEW_OMEGA, alpha=LONG_ALPHA)
        for tw in twins:
            cnt, w = _weights(oracle, g, tw, FEW_OMEGA, alpha=LONG_ALPHA)
            assert cnt.size > 8 * 2 * 32 and (cnt <= 2).sum() > cnt.size // 2   # more than two tiles per wave, mostly 1-2 walks
            assert int(w.max()) + 1 < WPACK_MAXW
        # the same case through a large epsilon: few walks per item again, every weight past the packed word
        rmax, omega = oracle.fora_setting(g.n, g.m, 8.0, alpha=LONG_ALPHA)
        _load_raw(engine, g, LONG_ALPHA, rmax, omega)
        _same_as_twin(engine, oracle, g, srcs, rmax, omega, alpha=LONG_ALPHA)
    finally:
        engine.reset_options()
        engine.set_graph(g.n, g.m, g.row_ptr, g.col)


@pytest.mark.parametrize("opt", [False, True])
def test_zero_degree_nodes(engine, oracle, small_dangling, opt):
    g = small_dangling
    rmax, omega = _load(engine, g, opt=opt)
    dang = np.flatnonzero(g.deg == 0)
    # sources with a dangling out-neighbour: their walks reach out-degree 0 at the first step; and one dangling source
    near = [v for v in np.flatnonzero(g.deg > 0) if np.isin(g.col[g.row_ptr[v]:g.row_ptr[v + 1]], dang).any()][:3]
    assert len(near) == 3 and dang.size
    srcs = [near[0], int(dang[1]), near[1], near[2]]
    _, st, twins = _same_as_twin(engine, oracle, g, srcs, rmax, omega, opt=opt)
    assert st[1]["dangling_source"] == 1 and st[1]["n_walks"] == 0 and st[0]["n_walks"] > 0
    for i in (0, 2, 3):
        assert twins[i][0][dang].any()                                      # mass did end on dangling nodes


@pytest.mark.parametrize("opt", [False, True])
def test_two_cycle_with_two_dangling_nodes(engine, oracle, opt):
    """4 nodes, every one a hub record (n <= 256), two of them with out-degree 0; every start in one batch."""
    g = oracle.Graph.from_edges(4, 4, np.array([0, 1, 0, 1], np.int32), np.array([1, 0, 2, 3], np.int32))
    assert list(g.deg) == [2, 2, 0, 0]
    for rmax, omega in ((0.3, 4000.0), (0.3, 1.0e6)):                        # weights past and inside the packed word
        _load_raw(engine, g, 0.2, rmax, omega, opt=opt)
        _same_as_twin(engine, oracle, g, [0, 1, 2, 3], rmax, omega, opt=opt)


def test_weights_that_do_not_fit_the_packed_word(engine, oracle, tiny_dangling):
    """omega just under 2^18 and a small rmax: items of few walks carry less than the average weight, so one batch has
    weights on both sides of WPACK_MAXW; then the default parameters of this graph (omega = 165 881: every weight past it)."""
    g = tiny_dangling
    srcs = pick_sources(g, 3, 413)
    rmax, omega = 1e-5, 250000.0
    _load_raw(engine, g, 0.2, rmax, omega)
    _, _, twins = _same_as_twin(engine, oracle, g, srcs, rmax, omega)
    over = under = 0
    for tw in twins:
        cnt, w = _weights(oracle, g, tw, omega)
        over += int((w + 1 >= WPACK_MAXW).sum())
        under += int((w + 1 < WPACK_MAXW).sum())
    assert over > 0 and under > 0, (over, under)
    rmax, omega = _load(engine, g)
    _, _, twins = _same_as_twin(engine, oracle, g, srcs, rmax, omega)
    cnt, w = _weights(oracle, g, twins[0], omega)
    assert (w >= WPACK_MAXW).all()


def test_full_buckets(engine, oracle, small_dangling):
    """One workgroup per slot and sub-buckets of 64 results (the smallest the plan allows): the stage's flush finds its
    bucket full and adds the rest by direct atomics.  The engine keeps no count of these, so the twin shows that a bucket
    must overflow: every node behind the hub records that walks end at sends at least one result, and they share nbx bins."""
    g = small_dangling
    engine.set_option("xb", 1)
    engine.set_option("bkcap", 8)
    try:
        rmax, omega = _load(engine, g)
        srcs = pick_sources(g, 3, 414)
        r0 = engine.get_option("bucket_retries")
        _, _, twins = _same_as_twin(engine, oracle, g, srcs, rmax, omega)
        assert engine.get_option("bucket_retries") == r0                    # (the capacity was not raised on the way)
        hubs = _dg_hub_set(g)
        nbx_max = max(2, ((g.n + 256 * 64) // 64 + 127) // 128)             # 64-id blocks behind the hubs, class padding included, 128 per bin
        for s, (want, _, _) in zip(srcs, twins):
            push = oracle.twin_push(g, int(s), rmax)
            ends = np.flatnonzero(want > push["reserve"])                   # nodes that walks ended at
            behind = [v for v in ends.tolist() if v not in hubs]
            assert len(behind) > 64 * nbx_max, (len(behind), nbx_max)
            cnt, w = _weights(oracle, g, (want, push["residue"], dict(rsum_fix=push["rsum_fix"])), omega)
            assert int(w.max()) + 1 < WPACK_MAXW                            # staged, not sent by the over-weight path
    finally:
        engine.reset_options()
        engine.set_graph(g.n, g.m, g.row_ptr, g.col)


@pytest.mark.parametrize("walk_dg,dg_hubs", [(1, 0), (2, 0), (2, 64), (2, 1024), (1, 1024)])
def test_variants(engine, oracle, small_dangling, walk_dg, dg_hubs):
    g = small_dangling
    engine.set_option("walk_dg", walk_dg)
    engine.set_option("dg_hubs", dg_hubs)
    try:
        for opt in (False, True):
            rmax, omega = _load(engine, g, opt=opt)
            srcs = list(pick_sources(g, 3, 415)) + list(pick_sources(g, 1, 416, want_dangling=True))
            _same_as_twin(engine, oracle, g, srcs, rmax, omega, opt=opt)
    finally:
        engine.reset_options()
        engine.set_graph(g.n, g.m, g.row_ptr, g.col)


@pytest.mark.parametrize("walk_dg", [1, 2])
def test_index_cut_to_a_third(engine, oracle, small_dangling, walk_dg):
    """A third of every node's indexed walks: k_walk_idx fills the buckets through the shared stage, the online two
    thirds follow through k_walk_dg in the same query."""
    g = small_dangling
    engine.set_option("walk_dg", walk_dg)
    try:
        rmax, omega = _load(engine, g)
        engine.build_index()
        rw_idx, off, cnt = engine.get_index()
        third = (cnt // 3).astype(cnt.dtype)
        engine.set_index(rw_idx, off, third)
        srcs = pick_sources(g, 3, 417)
        _, st, twins = _same_as_twin(engine, oracle, g, srcs, rmax, omega, index=(rw_idx, off, third))
        for s in st:
            assert 0 < s["n_idx_hit"] < s["n_walks"]
    finally:
        engine.clear_index()
        engine.reset_options()
        engine.set_graph(g.n, g.m, g.row_ptr, g.col)
