"""The line-aligned flush of k_walk_dg's result stages (options "walk_flush_align" = 0 / 8 / 16 results per line and
"walk_flush_keep", the cap on what a stage carries over; fora_amd/csrc/fora_flush_plan.h, stage_flush<.., ONE, G>): a flush
stores whole aligned lines of a sub-bucket and keeps the rest of every bin for the next one.  Only the order inside a
sub-bucket changes and k_accum adds integers, so every arm returns the twin's bits -- estimates and per-query statistics --
and therefore the bits of the arm that sends everything (walk_flush_align = 0).  The shapes are the smallest at which the
flush can go wrong:

  1. a handful of results per slot: no sub-bucket ever collects a line, everything leaves in the closing flush;
  2. ~20 k nodes, three or four bins, the graph's own parameters (~250 k walks a query): steady-state aligned flushes, the
     eight waves of a workgroup interleaving in the same sub-buckets; with four workgroups per slot and with one;
  3. the same with a cap of 16 (every flush takes the progress rule and the next re-aligns through head) and of 1;
  4. a third of the walk index in front of the online walks: k_walk_dg starts on non-zero, unaligned fills; and a top-k
     call of at least two rounds on the same graph;
  5. sub-buckets of 64 results (option "bkcap"): most results leave by the direct atomic, different ones per arm, same sums.

Every input property a case relies on is asserted from the twin, on the CPU."""
import numpy as np
import pytest

from conftest import pick_sources

pytestmark = pytest.mark.gpu
SEED = 0x464F5241
WPACK_MAXW = 1 << 44          # fora_kernels.h: weight bits of a staged result
STAGE = 384                   # DG_STAGE
ARMS = [(8, 0), (16, 0)]      # (walk_flush_align, walk_flush_keep)
PAIRS, RING = 6, 300
PAIR_RMAX, PAIR_OMEGA = 1e-5, 500000.0


@pytest.fixture(scope="module")
def mid(oracle):
    from fora_amd import synth
    n, m = 20000, 160000
    src, dst = synth.rmat_graph(n, m, 20260113, "rmat")
    return oracle.Graph.from_edges(n, m, src, dst)


@pytest.fixture(scope="module")
def pairs(oracle):
    """Two-cycles a <-> b apart from everything else, behind a ring of out-degree 2 that takes the hub records, and a node
    without edges.  A push from a goes back and forth until less than PAIR_RMAX is left on one of the two: one walk item of four or five walks."""
    src, dst = [], []
    for i in range(RING):
        src += [i, i]
        dst += [(i + 1) % RING, (i + 2) % RING]
    starts = []
    for k in range(PAIRS):
        a, b = RING + 2 * k, RING + 2 * k + 1
        src += [a, b]
        dst += [b, a]
        starts.append(a)
    n = RING + 2 * PAIRS + 1
    g = oracle.Graph.from_edges(n, len(src), np.array(src, np.int32), np.array(dst, np.int32))
    assert g.deg[n - 1] == 0 and n < 8192
    return g, np.array(starts + [n - 1], dtype=np.int32)


def _load(engine, g, raw=None, **kw):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    if raw:
        engine.set_params_raw(0.2, raw[0], raw[1], seed=SEED)
        return raw
    engine.set_params(seed=SEED, **kw)
    return engine.get_params()


def _arm(engine, align, keep):
    engine.set_option("walk_flush_align", align)
    engine.set_option("walk_flush_keep", keep)


def _restore(engine, g):
    engine.reset_options()
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)


STAT_KEYS = ("n_walks", "n_idx_hit", "ppr_sum_fix", "rsum_fix", "pops", "relax", "levels", "dangling_source")


def _stats(st):
    return [tuple(int(s[k]) for k in STAT_KEYS) for s in st]


def _twins(oracle, g, srcs, rmax, omega, **kw):
    return [oracle.twin_query(g, int(s), rmax, omega, seed=SEED, **kw) for s in srcs]


def _check(engine, oracle, g, srcs, twins, arms, with_idx=False):
    """Every arm against the twin and against walk_flush_align = 0, bit for bit."""
    _arm(engine, 0, 0)
    ppr0, res0, st0 = engine.query_fix(srcs, with_idx=with_idx)
    for i, (want, wres, wst) in enumerate(twins):
        assert (ppr0[i] == want).all() and (res0[i] == wres).all()
    for align, keep in arms:
        _arm(engine, align, keep)
        assert engine.get_option("walk_flush_align") == align and engine.get_option("walk_flush_keep") == keep
        engine.reset_timing()
        ppr, res, st = engine.query_fix(srcs, with_idx=with_idx)
        for i, (want, wres, wst) in enumerate(twins):
            bad = int((ppr[i] != want).sum())
            print("align", align, "keep", keep, "source", int(srcs[i]), "walks", wst["n_walks"], "differing", bad)
            assert bad == 0 and (res[i] == wres).all()
            assert st[i]["n_walks"] == wst["n_walks"] and st[i]["n_idx_hit"] == wst["n_idx_hit"]
            assert st[i]["ppr_sum_fix"] == int(want.sum(dtype=np.uint64))
        assert (ppr == ppr0).all() and (res == res0).all() and _stats(st) == _stats(st0)
        assert engine.timing()["walk_steps"] == sum(t[2]["walk_steps"] for t in twins)


def test_nothing_but_the_closing_flush(engine, oracle, pairs):
    g, srcs = pairs
    try:
        _load(engine, g, raw=(PAIR_RMAX, PAIR_OMEGA))
        twins = _twins(oracle, g, srcs, PAIR_RMAX, PAIR_OMEGA)
        staged = 0
        for want, res, st in twins[:-1]:
            _, cnt = oracle.twin_walk_counts(g, res, st["rsum_fix"], PAIR_OMEGA)
            nz = cnt > 0
            assert 1 <= st["n_walks"] < 8                                   # never a line of 8 in any sub-bucket
            assert int((res[nz] // cnt[nz]).max()) + 1 < WPACK_MAXW         # and every result goes through the wave's stage
            staged += st["n_walks"]
        assert staged >= PAIRS and twins[-1][2]["n_walks"] == 0            # (the node without edges: no walk at all)
        _check(engine, oracle, g, srcs, twins, ARMS + [(8, 1)])
    finally:
        _restore(engine, g)


@pytest.mark.parametrize("xb", [4, 1])
def test_steady_state_and_progress_rule(engine, oracle, mid, xb):
    g = mid
    try:
        engine.set_option("xb", xb)
        rmax, omega = _load(engine, g, epsilon=0.5)
        srcs = np.concatenate([pick_sources(g, 3, 41), pick_sources(g, 1, 42, want_dangling=True)])
        twins = _twins(oracle, g, srcs, rmax, omega)
        nbins = (g.n + 8191) // 8192
        assert nbins == 3
        for want, res, st in twins[:3]:
            _, cnt = oracle.twin_walk_counts(g, res, st["rsum_fix"], omega)
            nz = cnt > 0
            assert int((res[nz] // cnt[nz]).max()) + 1 < WPACK_MAXW         # staged results
            # dozens of flushes per wave: 8 or 32 waves per slot (the plan's 128 workgroups would leave a wave ~270 walks,
            # fewer than one flush), stages of 384
            assert st["n_walks"] > 32 * 20 * STAGE
        # cap 16 and cap 1: a flush keeps up to 7 (15) results a bin, so nearly every flush is a full one and the next
        # re-aligns; cap 0 (half the stage, 192) is never reached with four bins
        _check(engine, oracle, g, srcs, twins, ARMS + [(8, 16), (16, 16), (8, 1)])
    finally:
        _restore(engine, g)


def test_unaligned_starting_fills_and_topk_rounds(engine, oracle, mid):
    g = mid
    try:
        engine.set_option("xb", 2)      # (16 waves per slot: thousands of online walks a wave)
        rmax, omega = _load(engine, g, epsilon=0.5)
        srcs = pick_sources(g, 3, 43)
        engine.build_index()
        rw, off, cnt = engine.get_index()
        cnt3 = cnt // 3
        engine.set_index(rw, off, cnt3)
        twins = _twins(oracle, g, srcs, rmax, omega, index=(rw, off, cnt3))
        for want, res, st in twins:
            assert 0 < st["n_idx_hit"] < st["n_walks"] - 16 * 10 * STAGE    # indexed results in the buckets, online walks behind them
        _check(engine, oracle, g, srcs, twins, ARMS + [(8, 16)], with_idx=True)
        # top-k: every round runs the walk kernels again on the same workspace
        engine.clear_index()
        engine.set_params(epsilon=0.5, opt=True, seed=SEED)
        want = [oracle.twin_topk_query(g, int(s), 50, 0.5, seed=SEED) for s in srcs[:2]]
        assert max(w[2] for w in want) >= 2
        for align, keep in [(0, 0)] + ARMS + [(8, 16)]:
            _arm(engine, align, keep)
            ids, sc, rounds = engine.topk(srcs[:2], 50, epsilon=0.5)
            for i, (wid, wsc, wr, _) in enumerate(want):
                assert rounds[i] == wr and (ids[i] == wid).all() and (sc[i] == wsc).all(), (align, keep, i)
    finally:
        _restore(engine, g)


def test_sub_buckets_of_64_results(engine, oracle, mid):
    g = mid
    try:
        engine.set_option("bkcap", 8)   # (plan_workspace: at least 64 results a sub-bucket)
        engine.set_option("xb", 1)      # one workgroup per slot: one sub-bucket a bin takes all of a slot's results
        rmax, omega = _load(engine, g, epsilon=0.5)
        srcs = pick_sources(g, 2, 44)
        twins = _twins(oracle, g, srcs, rmax, omega)
        assert min(t[2]["n_walks"] for t in twins) > 100 * 64               # far more results than the sub-buckets hold
        _check(engine, oracle, g, srcs, twins, ARMS + [(8, 16)])
    finally:
        _restore(engine, g)
