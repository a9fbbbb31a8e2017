"""k_walk_dg with its per-wave LDS compacted (one 32-bit bin array per wave instead of two, tiles of 16 walk items, 16-bit
tile prefix sums) and the freed LDS spent on a stage of 384 results per wave -- against the twin, bit for bit, walk-step
counts included (test_walk_dg_loop_gpu._same_as_twin through test_walk_dg_balance_gpu._run), with the plan's workgroups
per slot and again with one (xb = 1).  The cases are the shapes at which the new layout can go wrong:

  - most of a flush in one bin, then in the next: the bin array holds counts, then stage offsets, then sub-bucket offsets
    less stage offsets, one after the other in the same words;
  - a sub-bucket that grows past 65 535 results (its offsets must stay 32 bits wide), and the same slot with sub-buckets of
    64 results, where nearly everything leaves through the overflow path;
  - slots of 0, 1, T - 1, T, T + 1 and 2 T + 1 walk items for the tile size T = 16, fewer tiles than waves; a heavy node
    whose items fill several tiles;
  - the other walk types: weights that do not fit the packed word, --opt (the NZH instantiations), long walks that outlive
    their tile, a third of the index;
  - a wave whose staged results end one short of, at, and one past the flush threshold of the 384-entry stage.

Every input property a case relies on is asserted from the twin, on the CPU."""
import numpy as np
import pytest

from conftest import pick_sources
from test_walk_dg_balance_gpu import (STAR_A, STAR_B, STAR_C, STAR_OMEGA, STAR_RMAX, STAR_S, STAR_Z, WALK_SEG, _both_grids,
                                      _online, _run, star)  # noqa: F401  (star: the hand-made graph's fixture)
from test_walk_dg_loop_gpu import FEW_OMEGA, FEW_RMAX, LONG_ALPHA, SEED, WPACK_MAXW, _dg_hub_set, _load_raw, _weights

pytestmark = pytest.mark.gpu
NW, T, STAGE = 8, 16, 384     # fora_kernels.h: waves per workgroup, items per wave's tile (DG_TILE / NW), DG_STAGE
FLUSH_AT = STAGE - 64 + 1     # stage_emit flushes once the wave's count has passed STAGE - 64


def _bucket_bins(g):
    """Bin of every node in WalkDG bucket order (-1: a hub record), and the number of bins: make_walk_dg of fora_tables.h --
    hubs first, then the out-degree classes by descending degree and ascending id, each padded to whole blocks, 64-id
    blocks dealt round-robin to nbx bins."""
    deg = np.asarray(g.deg).astype(np.int64)
    order = np.argsort(-deg, kind="stable")
    H = len(_dg_hub_set(g))
    ts = 6
    while ((g.n + 256 * (1 << ts)) >> ts) > 8192:
        ts += 1
    ids = np.full(g.n, -1, dtype=np.int64)
    ids[order[:H]] = np.arange(H)
    nxt, i = H, H
    while i < g.n:
        j = i
        while j < g.n and deg[order[j]] == deg[order[i]]:
            j += 1
        ids[order[i:j]] = nxt + np.arange(j - i)
        nxt += ((j - i + (1 << ts) - 1) >> ts) << ts
        i = j
    nbx = max(2, ((nxt - H + 63) // 64 + 127) // 128)
    return np.where(ids >= H, ((ids - H) >> 6) % nbx, -1), nbx


def _results_per_bin(oracle, g, s, twin, rmax, omega):
    """Bounds (lower, upper) of the walk results of a twin query that end in every bin: the mass the walks added over the
    largest and over the smallest weight a walk carries."""
    want, res, st = twin
    push = oracle.twin_push(g, int(s), rmax)
    _, w = _weights(oracle, g, twin, omega)
    bins, nbx = _bucket_bins(g)
    added = (want - push["reserve"]).astype(np.float64)
    mass = np.array([added[bins == b].sum() for b in range(nbx)])
    return mass / float(int(w.max()) + 1), mass / float(int(w.min())), nbx


def _assert_heavy_centre(cnt, items):
    assert cnt[STAR_C] >= 3 * T * WALK_SEG, int(cnt[STAR_C])                  # the centre's items fill several tiles
    assert items > 16 * NW * T                                                # a workgroup's tickets pass NW with 16 workgroups too


def test_most_of_a_flush_in_one_bin_then_in_the_next(engine, oracle, star):
    def body():
        _load_raw(engine, star, 0.2, STAR_RMAX, STAR_OMEGA)
        _, twins = _run(engine, oracle, star, [STAR_S], STAR_RMAX, STAR_OMEGA)
        cnt, items = _online(oracle, star, twins[0], STAR_OMEGA)
        _assert_heavy_centre(cnt, items)
        assert int(_weights(oracle, star, twins[0], STAR_OMEGA)[1].max()) + 1 < WPACK_MAXW   # staged results
        per_bin, _, nbx = _results_per_bin(oracle, star, STAR_S, twins[0], STAR_RMAX, STAR_OMEGA)
        print("results per bin >=", per_bin, "of", int(cnt.sum()), "walks")
        # two or three bins, an even and an odd one among them, each with more than a quarter of the staged results: a flush of
        # more than STAGE - 64 results holds well past 64 of each
        assert 2 <= nbx <= 3 and (per_bin[:2] > 0.25 * per_bin.sum()).all() and per_bin.sum() > 0.3 * cnt.sum()
        assert 0.25 * (STAGE - 64) > 64

    _both_grids(engine, star, body)


@pytest.mark.parametrize("bkcap", [1 << 18, 8])
def test_sub_bucket_past_65535(engine, oracle, star, bkcap):
    """One workgroup per slot and twice STAR_OMEGA: ~456 000 walks for the centre, more than 65 535 results in one
    sub-bucket.  bkcap 2^18: nothing overflows; bkcap 8 (sub-buckets of 64): nearly everything does."""
    g, omega = star, 2 * STAR_OMEGA
    engine.set_option("xb", 1)
    engine.set_option("bkcap", bkcap)
    try:
        _load_raw(engine, g, 0.2, STAR_RMAX, omega)
        r0 = engine.get_option("bucket_retries")
        _, twins = _run(engine, oracle, g, [STAR_S], STAR_RMAX, omega)
        assert engine.get_option("bucket_retries") == r0
        assert int(_weights(oracle, g, twins[0], omega)[1].max()) + 1 < WPACK_MAXW
        per_bin, at_most, _ = _results_per_bin(oracle, g, STAR_S, twins[0], STAR_RMAX, omega)
        print("results per bin >=", per_bin, "<=", at_most)
        assert per_bin.max() > 1.2 * 65535
        assert at_most.max() < bkcap or bkcap == 8                            # (2^18: every result has its place in the sub-bucket)
    finally:
        engine.reset_options()
        engine.set_graph(g.n, g.m, g.row_ptr, g.col)


# Fans: source s_k has one edge to each of k leaves, a leaf has its one edge back to s_k, and p_k has its one edge to s_k.
# The push goes back and forth between s_k and its leaves, every hop leaving 0.8 of the mass, until the sender's residue
# per edge is under rmax: after a hop from s_k the k leaves hold all the residue -- k walk items of a few dozen walks.
# Starting at p_k instead of s_k moves the hop count by one, so for every rmax one of the two starts ends on the leaves.
# 300 ring nodes of out-degree 2 take the hub records (with the sources of out-degree > 2), so the leaves stay behind them;
# Z has no edges.
FAN_KS = (1, T - 1, T, T + 1, 2 * T + 1)
FAN_RING = 300
FAN_RMAX = 1e-4               # (a leaf is left with ~9e-5: 25-29 walks at FEW_OMEGA, weights inside the packed word)


@pytest.fixture(scope="module")
def fans(oracle):
    src, dst, entry, nxt = [], [], {}, FAN_RING
    for i in range(FAN_RING):
        src += [i, i]
        dst += [(i + 1) % FAN_RING, (i + 2) % FAN_RING]
    for k in FAN_KS:
        s, p = nxt, nxt + 1
        leaves = list(range(nxt + 2, nxt + 2 + k))
        nxt += 2 + k
        src += [p] + [s] * k + leaves
        dst += [s] + leaves + [s] * k
        entry[k] = (s, p)
    z, n = nxt, nxt + 1
    g = oracle.Graph.from_edges(n, len(src), np.array(src, np.int32), np.array(dst, np.int32))
    assert g.deg[z] == 0 and n > 256
    srcs = [z]
    for k in FAN_KS:                                                          # the start that leaves k items, by the twin
        for s in entry[k]:
            tw = oracle.twin_query(g, s, FAN_RMAX, FEW_OMEGA, seed=SEED)
            if _online(oracle, g, tw, FEW_OMEGA)[1] == k and int(_weights(oracle, g, tw, FEW_OMEGA)[1].max()) + 1 < WPACK_MAXW:
                srcs.append(s)
                break
        else:
            raise AssertionError(("no start leaves k items", k))
    return g, srcs


def test_slots_of_0_1_and_around_a_tile_of_items(engine, oracle, fans):
    g, srcs = fans

    def body():
        _load_raw(engine, g, 0.2, FAN_RMAX, FEW_OMEGA)
        st, twins = _run(engine, oracle, g, srcs, FAN_RMAX, FEW_OMEGA)
        items = [_online(oracle, g, tw, FEW_OMEGA)[1] for tw in twins]
        print("items per slot", items)
        assert items == [0] + list(FAN_KS)
        assert st[0]["dangling_source"] == 1 and st[0]["n_walks"] == 0
        assert max(items) < NW * T                                            # fewer tiles than one workgroup has waves

    _both_grids(engine, g, body)


def test_weights_past_the_packed_word(engine, oracle, tiny):
    def body():
        rmax, omega = oracle.fora_setting(tiny.n, tiny.m, 0.5)
        _load_raw(engine, tiny, 0.2, rmax, omega)
        srcs = pick_sources(tiny, 3, 511)
        _, twins = _run(engine, oracle, tiny, srcs, rmax, omega)
        for tw in twins:
            assert (_weights(oracle, tiny, tw, omega)[1] >= WPACK_MAXW).all()

    _both_grids(engine, tiny, body)


OPT_OMEGA = 400000.0


def test_no_zero_hop_walks(engine, oracle, tiny):
    """--opt: a node gets 0.8 of the walks, each with 1 / 0.8 of the weight -- omega 400 000 keeps them inside the packed word."""
    def body():
        _load_raw(engine, tiny, 0.2, FEW_RMAX, OPT_OMEGA, opt=True)
        srcs = pick_sources(tiny, 3, 512)
        _, twins = _run(engine, oracle, tiny, srcs, FEW_RMAX, OPT_OMEGA, opt=True)
        for tw in twins:
            cnt, w = _weights(oracle, tiny, tw, OPT_OMEGA, opt=True)
            assert cnt.size > 2 * NW * T and int(w.max()) + 1 < WPACK_MAXW    # more than two tiles per wave of one workgroup, staged

    _both_grids(engine, tiny, body)


def test_long_walks_outlive_tiles_of_16(engine, oracle, tiny):
    """Items of 1-2 walks of ~125 iterations each: a wave replaces its tile about every iteration while the walks of earlier
    tiles still run -- their self sums must not land in the new tile's items."""
    def body():
        _load_raw(engine, tiny, LONG_ALPHA, FEW_RMAX, FEW_OMEGA)
        srcs = pick_sources(tiny, 2, 513)
        _, twins = _run(engine, oracle, tiny, srcs, FEW_RMAX, FEW_OMEGA, alpha=LONG_ALPHA)
        for tw in twins:
            cnt, w = _weights(oracle, tiny, tw, FEW_OMEGA, alpha=LONG_ALPHA)
            assert cnt.size > 2 * NW * T and (cnt <= 2).sum() > cnt.size // 2 and int(w.max()) + 1 < WPACK_MAXW
            assert tw[2]["walk_steps"] > 150 * tw[2]["n_walks"]

    _both_grids(engine, tiny, body)


def test_a_third_of_the_index(engine, oracle, star):
    """The centre's online walks begin inside an item, behind ~98 items that are indexed whole."""
    g, state = star, {}

    def body():
        _load_raw(engine, g, 0.2, STAR_RMAX, STAR_OMEGA)
        if not state:
            engine.build_index()
            rw_idx, off, cnt = engine.get_index()
            state["idx"] = (rw_idx, off, (cnt // 3).astype(cnt.dtype))
        engine.set_index(*state["idx"])
        st, twins = _run(engine, oracle, g, [STAR_S, STAR_A], STAR_RMAX, STAR_OMEGA, index=state["idx"])
        assert 0 < st[0]["n_idx_hit"] < st[0]["n_walks"]
        cnt, items = _online(oracle, g, twins[0], STAR_OMEGA, idx_cnt=state["idx"][2])
        _assert_heavy_centre(cnt, items)
        assert 0 < state["idx"][2][STAR_C] and state["idx"][2][STAR_C] % WALK_SEG != 0

    try:
        _both_grids(engine, g, body)
    finally:
        engine.clear_index()


# The two-cycle A <-> B of the hand-made graph with FLUSH_RMAX leaves ONE item of a few hundred walks: its walks end where
# they started (summed in LDS: one result when the wave gives up its tile) or at the partner, which lies behind the hub
# records -- one staged result each, all in one wave.  The walks of an item are its node's walks 0 .. N - 1 whatever omega
# is, and N grows with omega: the omega at which the partner's results reach a given count is found on the CPU by bisection.
FLUSH_RMAX = 2e-3


def _flush_case(oracle, g, staged):
    """(omega, twin) at which the one wave's staged results -- the partner's plus the self sum -- number `staged`."""
    def results(omega):
        tw = oracle.twin_query(g, STAR_A, FLUSH_RMAX, omega, seed=SEED)
        cnt, w = _weights(oracle, g, tw, omega)
        assert cnt.size == 1 and int(cnt[0]) <= WALK_SEG and int(w[0]) + 1 < WPACK_MAXW, (cnt, omega)
        v = int(np.flatnonzero(tw[1])[0])
        p = STAR_B if v == STAR_A else STAR_A
        push = oracle.twin_push(g, STAR_A, FLUSH_RMAX)
        at_p, at_v = int(tw[0][p] - push["reserve"][p]) // int(w[0]), int(tw[0][v] - push["reserve"][v]) // int(w[0])
        assert at_p + at_v == int(cnt[0]) and at_v > 0
        return at_p + 1, tw

    lo, hi = 270000.0, 500000.0                                               # (weights fit the packed word from omega = 2^18 on)
    assert results(lo)[0] < staged <= results(hi)[0]
    while hi - lo > 1e-3:
        mid = 0.5 * (lo + hi)
        if results(mid)[0] >= staged:
            hi = mid
        else:
            lo = mid
    got, tw = results(hi)
    assert got == staged, (got, staged)
    return hi, tw


@pytest.mark.parametrize("staged", [FLUSH_AT - 1, FLUSH_AT, FLUSH_AT + 1])
def test_flush_threshold_of_one_wave(engine, oracle, star, staged):
    g = star
    hubs = _dg_hub_set(g)
    assert STAR_A not in hubs and STAR_B not in hubs
    omega, _ = _flush_case(oracle, g, staged)
    print("staged", staged, "omega", omega)

    def body():
        _load_raw(engine, g, 0.2, FLUSH_RMAX, omega)
        _run(engine, oracle, g, [STAR_A], FLUSH_RMAX, omega)

    _both_grids(engine, g, body)


def test_three_workgroups_per_cu(engine, tiny):
    """The occupancy query for the launch's own instantiation and dynamic LDS size: 34 624 B static + tables is between a
    quarter and a third of the CU's 160 KB, and 8-wave workgroups at 7 waves per SIMD (106 SGPRs) come to three as well."""
    _load_raw(engine, tiny, 0.2, FEW_RMAX, FEW_OMEGA)
    assert engine.get_option("walk_dg_wgs_per_cu") == 3
