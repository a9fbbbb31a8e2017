"""The hand-out of tiles inside a k_walk_dg workgroup against the twin, bit for bit: a workgroup's waves take its tiles of
32 walk items by ticket (fora_consts.h: dg_ticket_tile), whoever runs out of walks first, instead of every eighth tile
each.  The cases are the shapes at which such a hand-out can go wrong: slots with fewer tiles than waves (most waves'
first ticket is already past the end), one node whose walks fill several whole tiles among items of two walks (a wave
stays on one tile while the others drain the rest), slots of every kind in one batch, the other instantiations, and
full result buckets (a workgroup still fills its own sub-buckets with its own tiles' results, in whatever order).

Every case also compares the engine's count of walk steps with the twin's: a tile run twice, or not at all, by a
weight-free walk would show there even where the sums happen to agree."""
import numpy as np
import pytest

from test_walk_dg_loop_gpu import FEW_OMEGA, FEW_RMAX, WPACK_MAXW, _dg_hub_set, _load_raw, _same_as_twin, _weights

pytestmark = pytest.mark.gpu
NW, WT, SUB = 8, 32, 16       # fora_kernels.h: waves per workgroup, items per tile; the plan's workgroups per slot
WALK_SEG = 1024               # walks per item at most (k_walk_alloc)

# The hand-made graph.  Source S has STAR_M parallel edges to the centre C and one to each light node; C has STAR_R
# parallel edges to each light node; a light node has its one edge to C.  With STAR_RMAX the source is pushed once and
# nobody else (C: 0.76 / 144 000 per edge, a light node: 6.4e-6, both under 7e-6), so C is left with 0.76 of the mass and
# each light node with 6.4e-6: at omega = 300 000 that is ~228 000 walks for C -- 223 consecutive items of 1024, seven
# tiles' worth starting inside a tile, since ~1000 light items come first -- and 2 walks for every light node, 6219 items
# = 195 tiles: more than SUB * NW, so a workgroup's tickets reach their second lap.  Weights are 2^62 / omega < 2^44:
# the results go through the wave's stage.  A and B are a two-cycle apart from the rest (pushed until 6e-6 is left: one
# item of one or two walks), Z has no edges.
STAR_LIGHT, STAR_M, STAR_R = 6000, 119000, 24
STAR_C, STAR_S, STAR_A, STAR_B, STAR_Z = 1000, 3000, 4000, 4001, 5000
STAR_RMAX, STAR_OMEGA = 7e-6, 300000.0


@pytest.fixture(scope="module")
def star(oracle):
    n = STAR_LIGHT + 5
    special = np.array([STAR_C, STAR_S, STAR_A, STAR_B, STAR_Z])
    light = np.setdiff1d(np.arange(n), special)
    assert light.size == STAR_LIGHT
    src = np.concatenate([np.full(STAR_M, STAR_S), np.full(light.size, STAR_S), np.repeat(STAR_C, STAR_R * light.size), light,
                          [STAR_A, STAR_B]])
    dst = np.concatenate([np.full(STAR_M, STAR_C), light, np.tile(light, STAR_R), np.full(light.size, STAR_C),
                          [STAR_B, STAR_A]])
    g = oracle.Graph.from_edges(n, src.size, src.astype(np.int32), dst.astype(np.int32))
    assert g.deg[STAR_S] == STAR_M + STAR_LIGHT and g.deg[STAR_C] == STAR_R * STAR_LIGHT and g.deg[STAR_Z] == 0
    return g


def _online(oracle, g, twin, omega, alpha=0.2, opt=False, idx_cnt=None):
    """Per node, the walks of a twin query that k_walk_dg runs (those the index does not hold), and the slot's item count."""
    _, res, st = twin
    _, cnt = oracle.twin_walk_counts(g, res, st["rsum_fix"], omega, alpha=alpha, opt=opt)
    cnt = cnt.astype(np.int64)
    items = int(((cnt + WALK_SEG - 1) // WALK_SEG).sum())
    if idx_cnt is not None:
        cnt = cnt - np.minimum(cnt, idx_cnt.astype(np.int64))
    return cnt, items


def _run(engine, oracle, g, srcs, rmax, omega, **kw):
    """One batch against the twin, bit for bit, the walk-step count included."""
    engine.reset_timing()
    _, st, twins = _same_as_twin(engine, oracle, g, srcs, rmax, omega, **kw)
    got, want = engine.timing()["walk_steps"], sum(t[2]["walk_steps"] for t in twins)
    print("walk_steps", got, want)
    assert got == want
    return st, twins


def _both_grids(engine, g, body):
    """body() with the plan's SUB workgroups per slot, then with one."""
    try:
        body()
        engine.set_option("xb", 1)
        body()
    finally:
        engine.reset_options()
        engine.set_graph(g.n, g.m, g.row_ptr, g.col)


def _assert_heavy_centre(cnt, items):
    """The centre's walks fill at least 3 * WT consecutive items of 1024, and most other items have one or two walks."""
    assert cnt[STAR_C] >= 3 * WT * WALK_SEG, int(cnt[STAR_C])
    others = np.delete(cnt, STAR_C)
    others = others[others > 0]
    assert others.size > 4 * WT and (others <= 2).sum() > 0.9 * others.size, (others.size, int((others <= 2).sum()))
    assert items > NW * WT                                                    # more tiles than one workgroup has waves


def test_fewer_tiles_than_waves(engine, oracle, tiny, star):
    """Slots of one tile (the two-cycle of the hand-made graph: one item) and slots of 38 tiles (tiny, 1203 items of mostly
    1-2 walks) under SUB * NW = 128 waves, then under 8."""
    def one_tile():
        _load_raw(engine, star, 0.2, STAR_RMAX, STAR_OMEGA)
        _, twins = _run(engine, oracle, star, [STAR_A, STAR_B], STAR_RMAX, STAR_OMEGA)
        for tw in twins:
            cnt, items = _online(oracle, star, tw, STAR_OMEGA)
            assert 1 <= items <= WT and cnt.sum() > 0, items

    def few_tiles():
        _load_raw(engine, tiny, 0.2, FEW_RMAX, FEW_OMEGA)
        srcs = [int(np.flatnonzero(tiny.deg > 0)[k]) for k in (5, 77, 400)]
        _, twins = _run(engine, oracle, tiny, srcs, FEW_RMAX, FEW_OMEGA)
        for tw in twins:
            _, items = _online(oracle, tiny, tw, FEW_OMEGA)
            assert WT < items < SUB * NW * WT, items                          # more than one tile, fewer tiles than waves

    _both_grids(engine, star, one_tile)
    _both_grids(engine, tiny, few_tiles)


def test_one_heavy_node_among_light_ones(engine, oracle, star):
    def body():
        _load_raw(engine, star, 0.2, STAR_RMAX, STAR_OMEGA)
        _, twins = _run(engine, oracle, star, [STAR_S], STAR_RMAX, STAR_OMEGA)
        cnt, items = _online(oracle, star, twins[0], STAR_OMEGA)
        _assert_heavy_centre(cnt, items)
        assert items > SUB * NW * WT                                          # a workgroup's tickets pass NW also with SUB workgroups
        assert int(_weights(oracle, star, twins[0], STAR_OMEGA)[1].max()) + 1 < WPACK_MAXW   # staged results

    _both_grids(engine, star, body)


def test_three_kinds_of_slot_in_one_batch(engine, oracle, star):
    def body():
        _load_raw(engine, star, 0.2, STAR_RMAX, STAR_OMEGA)
        srcs = [STAR_Z, STAR_A, STAR_S, STAR_Z, STAR_B]
        st, twins = _run(engine, oracle, star, srcs, STAR_RMAX, STAR_OMEGA)
        items = [_online(oracle, star, tw, STAR_OMEGA)[1] for tw in twins]
        assert st[0]["dangling_source"] == 1 and st[0]["n_walks"] == 0 and items[0] == 0 and items[3] == 0
        assert 1 <= items[1] <= WT and 1 <= items[4] <= WT and items[2] > SUB * NW * WT, items

    _both_grids(engine, star, body)


def test_heavy_node_without_zero_hop_walks(engine, oracle, star):
    """--opt: the instantiation whose walks take their first step whatever the first random word says."""
    def body():
        _load_raw(engine, star, 0.2, STAR_RMAX, STAR_OMEGA, opt=True)
        _, twins = _run(engine, oracle, star, [STAR_S, STAR_A], STAR_RMAX, STAR_OMEGA, opt=True)
        _assert_heavy_centre(*_online(oracle, star, twins[0], STAR_OMEGA, opt=True))

    _both_grids(engine, star, body)


def test_heavy_node_behind_a_third_of_the_index(engine, oracle, star):
    """A third of every node's indexed walks: the centre's first ~98 items are indexed whole, one is split, and the online
    walks of the rest start past idx_n; a light node has one walk of each kind."""
    g = star
    state = {}

    def body():
        _load_raw(engine, g, 0.2, STAR_RMAX, STAR_OMEGA)
        if not state:
            engine.build_index()
            rw_idx, off, cnt = engine.get_index()
            state["idx"] = (rw_idx, off, (cnt // 3).astype(cnt.dtype))
        engine.set_index(*state["idx"])
        st, twins = _run(engine, oracle, g, [STAR_S], STAR_RMAX, STAR_OMEGA, index=state["idx"])
        assert 0 < st[0]["n_idx_hit"] < st[0]["n_walks"]
        cnt, items = _online(oracle, g, twins[0], STAR_OMEGA, idx_cnt=state["idx"][2])
        _assert_heavy_centre(cnt, items)
        assert 0 < state["idx"][2][STAR_C] and state["idx"][2][STAR_C] % WALK_SEG != 0   # the centre's online walks begin inside an item

    try:
        _both_grids(engine, g, body)
    finally:
        engine.clear_index()


def test_full_buckets_and_repeatability(engine, oracle, star):
    """One workgroup per slot and sub-buckets of 64 results: ~5700 light nodes behind the hub records share at most three bins, and about
    half of the centre's 228 000 walks end on them.  A workgroup's set of tiles is what it was, so its sub-buckets overflow
    as before: the capacity is not raised; and whichever wave ran which tile, the words are the same."""
    g = star
    engine.set_option("xb", 1)
    engine.set_option("bkcap", 8)
    try:
        _load_raw(engine, g, 0.2, STAR_RMAX, STAR_OMEGA)
        r0 = engine.get_option("bucket_retries")
        _, twins = _run(engine, oracle, g, [STAR_S, STAR_A], STAR_RMAX, STAR_OMEGA)
        assert engine.get_option("bucket_retries") == r0
        want = twins[0][0]
        # a bucket must overflow (as test_full_buckets shows it): every node behind the hub records that walks end at sends at
        # least one result, and they share at most nbx_max bins of 64 slots in the one workgroup's sub-buckets
        hubs = _dg_hub_set(g)                                               # S, C and the 254 light nodes of lowest id
        nbx_max = max(2, ((g.n + 256 * 64) // 64 + 127) // 128)
        push = oracle.twin_push(g, STAR_S, STAR_RMAX)
        ends = np.flatnonzero(want > push["reserve"])                       # nodes that walks ended at
        behind = [v for v in ends.tolist() if v not in hubs]
        assert len(behind) > 64 * nbx_max, (len(behind), nbx_max)
        assert int(_weights(oracle, g, twins[0], STAR_OMEGA)[1].max()) + 1 < WPACK_MAXW   # staged, not sent by the over-weight path
        a = engine.query_fix(np.array([STAR_S, STAR_A], dtype=np.int32))
        b = engine.query_fix(np.array([STAR_S, STAR_A], dtype=np.int32))
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[0][0] == want).all()
        assert engine.get_option("bucket_retries") == r0
    finally:
        engine.reset_options()
        engine.set_graph(g.n, g.m, g.row_ptr, g.col)
