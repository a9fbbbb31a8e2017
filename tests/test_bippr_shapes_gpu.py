"""The backward push and the BiPPR combine away from the one point test_bippr_gpu.py checks them at: deep pushes, other
alphas, random graph shapes, every pairing of the tier and chunk options, the exact tier boundary, a hash table whose
probes collide and wrap, residues exactly on the pop threshold, wide and uneven batches, several chunks under the
combine, top-k with ties.  Everything is compared bit for bit with the Python-int twin of tests/bippr_ref.py; which targets
and sources a case uses follows from the graph and the twin alone, and every case asserts from the twin (or the returned
counters) that it ran what it claims to run."""
import functools
import math
import os
import re

import numpy as np
import pytest

import bippr_ref as br
from conftest import pick_sources

pytestmark = pytest.mark.gpu
SEED = 0x464F5241
EPS = 0.5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP_DEFAULT, CAP_MAX, TAB_BITS = 1024, 1536, 11  # fora_bwd.h, asserted by test_header_constants
STAT_KEYS = ("targets", "pops", "relax", "entries", "levels", "global_targets", "chunks")


def test_header_constants():
    """The cases below are built around these values of fora_bwd.h; if the table changes they must be rebuilt."""
    hdr = open(os.path.join(ROOT, "fora_amd", "csrc", "fora_bwd.h")).read()
    assert re.search(r"constexpr int BWD_TAB_BITS = %d;" % TAB_BITS, hdr)
    assert re.search(r"constexpr uint32_t BWD_CAP_MAX = %d;" % CAP_MAX, hdr)
    assert re.search(r"constexpr uint32_t BWD_CAP_DEFAULT = %d;" % CAP_DEFAULT, hdr)
    assert len(re.findall(r"\* 0x9E3779B1u\) >> \(32 - BWD_TAB_BITS\)", hdr)) == 2  # the insert and the target's own slot
    assert re.search(r"h = \(h \+ 1\) & \(BWD_TAB - 1\);", hdr)                      # linear probing, wrapping
    assert int(br.slot_of(1, TAB_BITS)) == 0x9E3779B1 >> (32 - TAB_BITS)


def _load(engine, g, alpha):
    engine.clear_index()
    engine.reset_options()
    engine.set_batch(0)
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(alpha=alpha, epsilon=EPS, seed=SEED)


def _expected(g, targets, rmax, alpha):
    """Dense reserve / residue rows, the summed counters and the support sizes of the twin's pushes, one per target."""
    nt = len(targets)
    rsv = np.zeros((nt, g.n), dtype=np.uint64)
    res = np.zeros((nt, g.n), dtype=np.uint64)
    pops = relax = entries = levels = 0
    supports, memo = [], {}
    for i, t in enumerate(targets):
        t = int(t)
        if t not in memo:
            memo[t] = br.twin_bwd_push_sparse(g, t, rmax, alpha)
        p, r, po, re_, lv = memo[t]
        if p:
            rsv[i, list(p)] = np.array(list(p.values()), dtype=np.uint64)
        res[i, list(r)] = np.array(list(r.values()), dtype=np.uint64)
        pops, relax, entries, levels = pops + po, relax + re_, entries + br.entries_of(p, r), max(levels, lv)
        supports.append(len(br.support_of(r)))
    return dict(reserve=rsv, residue=res, supports=supports,
                stats=dict(targets=nt, pops=pops, relax=relax, entries=entries, levels=levels))


def _expected_stats(want, nt, cap, chunk):
    eff = CAP_DEFAULT if cap is None else min(max(cap, 0), CAP_MAX)
    return dict(want["stats"], global_targets=nt if eff == 0 else br.targets_over_cap(want["supports"], eff),
                chunks=1 if chunk <= 0 else -(-nt // chunk))


def _push(engine, targets, rmax, want, cap=None, chunk=0):
    """One fora_hip_bwdpush_batch call under the two options; rows and counters must equal the twin's."""
    engine.reset_options()
    if cap is not None:
        engine.set_option("bwd_lds_cap", cap)
    engine.set_option("bwd_chunk", chunk)
    try:
        rsv, res, bwd = engine.bwdpush(np.asarray(targets, dtype=np.int32), rmax)
    finally:
        engine.reset_options()
    got = {k: bwd[k] for k in STAT_KEYS}
    exp = _expected_stats(want, len(targets), cap, chunk)
    assert got == exp, (cap, chunk, got, exp)
    bad = (rsv != want["reserve"]) | (res != want["residue"])
    assert not bad.any(), (cap, chunk, int(bad.sum()), np.flatnonzero(bad.any(axis=1))[:8].tolist())
    return bwd


@functools.lru_cache(maxsize=None)
def _widest(g, rmax, alpha, pool=0):
    """(target, support) of the widest push according to the twin: over every node of the graph (pool = 0), or over the
    `pool` nodes of largest two-hop in-degree and the `pool` of largest in-degree where n twin pushes are too many.  Ties
    go to the lowest id.  (The cache holds g, so its identity stays taken.)"""
    if pool:
        nnz = int(g.row_ptr[-1])
        indeg = np.bincount(g.col[:nnz], minlength=g.n)
        two_hop = np.bincount(g.col[:nnz], weights=indeg[np.repeat(np.arange(g.n), g.deg)], minlength=g.n)
        cand = sorted(set(np.argsort(-two_hop, kind="stable")[:pool].tolist()) | set(np.argsort(-indeg, kind="stable")[:pool].tolist()))
    else:
        cand = range(g.n)
    sup = [len(br.support_of(br.twin_bwd_push_sparse(g, t, rmax, alpha)[1])) for t in cand]
    best = max(range(len(sup)), key=lambda i: (sup[i], -cand[i]))
    return int(cand[best]), sup[best]


def _sample(g, seed, widest, count=64):
    """The targets of a sampled case: the target of the widest push (_widest), the node of largest in-degree, a node
    without in-edges and a dangling node (where the graph has one) at the end of the list, random distinct nodes in
    front, `count` in all."""
    indeg = np.bincount(g.col, minlength=g.n)
    no_in, dang = np.flatnonzero(indeg == 0), np.flatnonzero(g.deg == 0)
    special = [int(widest)] + [v for v in [int(indeg.argmax())] if v != widest]
    if no_in.size:
        special.append(int(next(v for v in no_in[no_in.size // 2:].tolist() if v not in special)))
    if dang.size:
        special.append(int(next(v for v in dang.tolist() if v not in special)))
    rng = np.random.Generator(np.random.PCG64(seed))
    rest = [v for v in rng.permutation(g.n).tolist() if v not in special][:max(0, count - len(special))]
    return np.array(rest + special, dtype=np.int32)


# ---------------------------------------------------------------------------------------------- backward push
@pytest.mark.parametrize("alpha", [0.05, 0.2, 0.85])
@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling"])
def test_deep_pushes_bit_exact(engine, request, gname, alpha):
    """64 targets per case: the target whose push is the widest of all n according to the twin (ranked at rmax 1e-2, where
    n twin pushes are cheap; deeper, many pushes cover all they can reach and tie), the node of largest
    in-degree, one without in-edges and (tiny_dangling) a dangling one, the rest random."""
    g = request.getfixturevalue(gname)
    _load(engine, g, alpha)
    widest, wsup = _widest(g, 1e-2, alpha)
    targets = _sample(g, 501, widest)
    indeg = np.bincount(g.col, minlength=g.n)
    assert targets.size == np.unique(targets).size == 64 and int(indeg.argmax()) in targets and (indeg[targets] == 0).any()
    assert widest in targets and wsup == max(_expected(g, targets, 1e-2, alpha)["supports"])  # no target of the graph is wider
    assert gname == "tiny" or (g.deg[targets] == 0).any()
    deepest = widest = 0
    for rmax in (1e-2, 1e-3, 1e-4):
        want = _expected(g, targets, rmax, alpha)
        _push(engine, targets, rmax, want)
        _push(engine, targets, rmax, want, cap=0)
        deepest, widest = max(deepest, want["stats"]["levels"]), max(widest, max(want["supports"]))
        if rmax == 1e-4:  # under the default cap both tiers run
            assert 0 < br.targets_over_cap(want["supports"], CAP_DEFAULT) < targets.size
    # far past the 6 levels and the 437 nodes of BiPPR's own rmax (the twin's figures, not the GPU's)
    assert deepest >= {0.05: 50, 0.2: 20, 0.85: 4}[alpha] and widest > CAP_DEFAULT


def test_deep_pushes_small_graph(engine, small):
    g = small
    _load(engine, g, 0.2)
    rmax = 1e-3
    # n = 32 000: the widest of the likeliest candidates (largest in-degree, largest two-hop in-degree), ranked at 1e-2
    widest, wsup = _widest(g, 1e-2, 0.2, pool=24)
    targets = _sample(g, 502, widest)
    want = _expected(g, targets, rmax, 0.2)
    assert targets.size == np.unique(targets).size == 64 and widest in targets
    assert wsup == max(_expected(g, targets, 1e-2, 0.2)["supports"]) and wsup > CAP_MAX
    assert max(want["supports"]) > CAP_MAX and min(want["supports"]) <= CAP_DEFAULT
    _push(engine, targets, rmax, want)
    _push(engine, targets, rmax, want, cap=CAP_MAX, chunk=7)


@functools.lru_cache(maxsize=None)
def _option_case(g):
    """tiny_dangling at rmax 1e-3, alpha 0.2: the targets of test_deep_pushes_bit_exact, then duplicates of the first two
    and of the last three (special) ones, so the last chunks hold wide pushes (global on any small cap) next to the node
    without in-edges (a support of 1: on the LDS tier under every cap but 0)."""
    tg = _sample(g, 501, _widest(g, 1e-2, 0.2)[0])
    targets = np.concatenate([tg, tg[:2], tg[-3:]])
    return targets, _expected(g, targets, 1e-3, 0.2)


def _mixed_later_chunk(supports, cap, chunk):
    """A chunk after the first that holds a global-tier target and an LDS-tier one."""
    for t0 in range(chunk, len(supports), chunk):
        over = [s > cap for s in supports[t0:t0 + chunk]]
        if any(over) and not all(over):
            return True
    return False


def test_tier_and_chunk_options_combined(engine, tiny_dangling):
    g = tiny_dangling
    _load(engine, g, 0.2)
    targets, want = _option_case(g)
    nt = targets.size
    assert nt == 69 and np.unique(targets).size == 64
    for cap in (1, 40):
        assert _mixed_later_chunk(want["supports"], cap, 7)
    over = [br.targets_over_cap(want["supports"], cap) for cap in (CAP_MAX, CAP_DEFAULT, 40, 1)]
    assert 0 == over[0] < over[1] < over[2] <= over[3] < nt  # (supports here: 1, or 84 and more)
    for cap in (None, 0, 1, 40, CAP_MAX):
        for chunk in (0, 1, 7, nt - 1):
            bwd = _push(engine, targets, 1e-3, want, cap=cap, chunk=chunk)
            if chunk:
                assert bwd["chunks"] > 1


def test_exact_tier_boundary(engine, tiny_dangling):
    """A push of support S fits a table of S entries and not one of S - 1."""
    g = tiny_dangling
    _load(engine, g, 0.2)
    targets, want = _option_case(g)
    sup = want["supports"]
    fits = sorted({s for s in sup if s <= CAP_MAX})
    picks = sorted({fits[0], fits[1], fits[len(fits) // 3], fits[len(fits) // 2], fits[-2], fits[-1]})
    assert picks[0] == 1 and picks[-1] > CAP_DEFAULT and len(picks) >= 5
    for S in picks:
        # the whole call: global_targets == #{support > cap} is part of _push's comparison
        a = _push(engine, targets, 1e-3, want, cap=S)
        b = _push(engine, targets, 1e-3, want, cap=S - 1)
        assert b["global_targets"] - a["global_targets"] == (sup.count(S) if S > 1 else len(sup) - a["global_targets"])
        one = targets[[sup.index(S)]]
        w1 = _expected(g, one, 1e-3, 0.2)
        assert w1["supports"] == [S]
        assert _push(engine, one, 1e-3, w1, cap=S)["global_targets"] == 0
        assert _push(engine, one, 1e-3, w1, cap=S - 1)["global_targets"] == 1


#            n, kind, mean degree, alpha, rmax
_SHAPES = [(1, "uniform", 0.0, 0.2, 1e-4), (2, "pair", 1.5, 0.5, 1e-4), (37, "power", 6.0, 0.05, 1e-4),
           (64, "uniform", 0.7, 0.2, 1e-4), (65, "giant", 2.0, 0.85, 1e-4), (257, "power", 20.0, 0.2, 1e-2),
           (1000, "uniform", 6.0, 0.5, 1e-2), (2049, "giant", 2.0, 0.05, 1e-2), (4097, "power", 6.0, 0.2, 1e-3)]


def _shape_graph(oracle, n, kind, avg, seed):
    rng = np.random.Generator(np.random.PCG64(2000 + seed))
    m = int(n * avg)
    if kind == "pair":     # 0 -> 1 twice, 1 -> 0
        src, dst = np.array([0, 0, 1]), np.array([1, 1, 0])
    elif kind == "power":  # power-law sources and targets, duplicates kept
        src = np.minimum((n * rng.random(m) ** 3).astype(np.int64), n - 1)
        dst = np.minimum((n * rng.random(m) ** 2).astype(np.int64), n - 1)
    elif kind == "uniform":
        src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    else:                  # a few giant rows over a sparse background
        hubs = rng.integers(0, n, 3)
        src = np.concatenate([rng.integers(0, n, m // 2), rng.choice(hubs, m - m // 2)])
        dst = rng.integers(0, n, m)
    if n > CAP_MAX + 200:  # node n - 1 gets 1700 distinct in-neighbours: no table of the LDS tier holds its push
        src, dst = np.concatenate([src, np.arange(1700)]), np.concatenate([dst, np.full(1700, n - 1)])
    return oracle.Graph.from_edges(n, max(1, src.size), src.astype(np.int32), dst.astype(np.int32))


@pytest.mark.parametrize("seed", range(len(_SHAPES)))
def test_random_shapes_vs_twin(engine, oracle, seed):
    n, kind, avg, alpha, rmax = _SHAPES[seed]
    g = _shape_graph(oracle, n, kind, avg, seed)
    nnz = int(g.row_ptr[-1])
    indeg = np.bincount(g.col[:nnz], minlength=n)
    if kind in ("pair", "power"):  # duplicate edges are kept
        src = np.repeat(np.arange(n, dtype=np.int64), g.deg)
        assert np.unique(src * n + g.col[:nnz]).size < nnz
    if avg < 1:
        assert nnz < n
    if kind == "giant":
        assert g.deg.max() > 8 * max(1.0, avg)
    _load(engine, g, alpha)
    targets = np.arange(n, dtype=np.int32) if n <= 2100 else _sample(g, 700 + seed, _widest(g, rmax, alpha, pool=24)[0])
    targets = np.concatenate([targets, targets[:1]])  # and a duplicate
    want = _expected(g, targets, rmax, alpha)
    if n > 2100:
        assert _widest(g, rmax, alpha, pool=24)[1] == max(want["supports"])
    if n > CAP_MAX + 200:
        hub = n - 1
        assert indeg[hub] > CAP_MAX and hub == indeg.argmax() and want["supports"][targets.tolist().index(hub)] > CAP_MAX
    nt = targets.size
    _push(engine, targets, rmax, want)
    _push(engine, targets, rmax, want, cap=40, chunk=7)
    _push(engine, targets, rmax, want, cap=0, chunk=max(1, nt - 1))
    _push(engine, targets, rmax, want, cap=1, chunk=1)


def test_hash_collisions_and_wrap_around(engine, oracle):
    """In-neighbours picked by their home slot in the LDS table: 12 of the target's in-neighbours live in slots
    2040 .. 2047 (more than the 8 slots there are before the table's end: a probe has to wrap to slot 0), 250 share
    slot 1000, and 200 nodes one level further out share slot 2046 (a cluster that wraps by nearly 200 slots).  The
    multiplicative hash spreads consecutive ids evenly, n / 2048 to a slot, so a few hundred ids in one slot need
    n = 600 000."""
    test_header_constants()
    n = 600_000
    slot = br.slot_of(np.arange(n), TAB_BITS)
    assert slot.max() == (1 << TAB_BITS) - 1
    t = 12345
    end = np.flatnonzero((slot >= 2040) & (slot != 2046))
    end = end[end != t][:12]
    same = np.flatnonzero(slot == 1000)
    same = same[same != t][:250]
    far = np.flatnonzero(slot == 2046)
    far = far[far != t][:200]
    assert end.size == 12 and same.size == 250 and far.size == 200
    layer1 = np.concatenate([end, same])
    rng = np.random.Generator(np.random.PCG64(31))
    src = np.concatenate([layer1, far, rng.integers(0, n, 1500)])
    dst = np.concatenate([np.full(layer1.size, t), layer1[:far.size], rng.integers(0, n, 1500)])
    g = oracle.Graph.from_edges(n, src.size, src.astype(np.int32), dst.astype(np.int32))
    assert 1900 <= int(g.row_ptr[-1]) <= 2000
    alpha, rmax = 0.2, 1e-4
    targets = np.array([t, layer1[0], t, far[0], layer1[20]], dtype=np.int32)
    want = _expected(g, targets, rmax, alpha)
    keys = np.array(sorted(br.support_of(br.twin_bwd_push_sparse(g, t, rmax, alpha)[1])))
    home = br.slot_of(keys, TAB_BITS).astype(np.int64)
    assert keys.size == want["supports"][0] and 1 + 12 + 250 + 200 <= keys.size <= CAP_DEFAULT   # on the LDS tier by default
    assert (home >= 2040).sum() > 2048 - 2040                           # some probe wraps past the table's end
    assert np.bincount(home).max() >= 250 and (home == 2046).sum() >= 200
    assert want["stats"]["levels"] >= 3
    _load(engine, g, alpha)
    assert _push(engine, targets, rmax, want)["global_targets"] == 0
    assert _push(engine, targets, rmax, want, cap=CAP_MAX, chunk=2)["global_targets"] == 0
    assert _push(engine, targets, rmax, want, cap=keys.size)["global_targets"] == 0
    assert _push(engine, targets, rmax, want, cap=keys.size - 1)["global_targets"] == 2
    assert _push(engine, targets, rmax, want, cap=0)["global_targets"] == targets.size


def test_pop_rule_on_the_threshold(engine, oracle):
    """The cases of test_bippr_cpu.py::test_pop_rule_on_the_threshold on both tiers: a residue of exactly
    floor(rmax * 2^60) stays, one ulp of rmax less and it pops."""
    n, src, dst, t, u = br.threshold_graph()
    g = oracle.Graph.from_edges(n, src.size, src, dst)
    alpha = 0.5
    _load(engine, g, alpha)
    cases = [(0.25, 1), (math.nextafter(0.25, 0), 2), (1.0, 0), (math.nextafter(1.0, 0), 1)]
    for rmax, pops in cases:
        want = _expected(g, [t], rmax, alpha)
        assert want["stats"]["pops"] == pops
        thr = math.floor(math.ldexp(rmax, 60))
        if rmax in (0.25, 1.0):  # equality on the threshold, in the twin's own residue
            assert int(want["residue"][0].max()) == thr
        for cap in (None, 0):
            _push(engine, [t], rmax, want, cap=cap)
            _push(engine, [t, u, 3, 2, t], rmax, _expected(g, [t, u, 3, 2, t], rmax, alpha), cap=cap, chunk=2)


# ---------------------------------------------------------------------------------------------- BiPPR estimate
@functools.lru_cache(maxsize=None)
def _pushes(g, rmax, alpha):
    """The twin's pushes of every node, their summed counters and support sizes.  (This cache and the ones below take the
    graph by identity and hold it.)"""
    pushes, pops, relax, entries, levels, supports = [], 0, 0, 0, 0, []
    for t in range(g.n):
        p, r, po, re_, lv = br.twin_bwd_push_sparse(g, t, rmax, alpha)
        pushes.append((p, r))
        pops, relax, entries, levels = pops + po, relax + re_, entries + br.entries_of(p, r), max(levels, lv)
        supports.append(len(br.support_of(r)))
    return dict(pushes=pushes, supports=supports,
                stats=dict(targets=g.n, pops=pops, relax=relax, entries=entries, levels=levels))


@functools.lru_cache(maxsize=None)
def _ends(engine, oracle, g, s, W, alpha, cpu):
    """Endpoints of the W walks of source s: from the CPU oracle (cpu=True) or from fora_hip_walks, which has its own
    parity test (the graph is loaded)."""
    if cpu:
        return np.array([oracle.walk(g, SEED, s, 0, s, j, alpha=alpha) for j in range(W)], dtype=np.int64)
    return engine.walks(s, 0, np.full(W, s, dtype=np.int32), np.arange(W, dtype=np.uint64)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _estimate(engine, oracle, g, s, rmax, W, alpha, cpu):
    return br.twin_bippr(g, s, rmax, W, _ends(engine, oracle, g, s, W, alpha, cpu), alpha, pushes=_pushes(g, rmax, alpha)["pushes"])


def _even_batch(nq, B):
    """Slots per batch of a call with nq sources under a batch limit of B.  A restatement of `static int even_batch(int nq,
    int B)` in fora_amd/csrc/fora_hip.hip, which walk_batches splits a call with: if that function changes, this one
    has to follow."""
    if nq <= B or B <= 0:
        return max(nq, 1)
    nbatch = -(-nq // B)
    return -(-nq // nbatch)


def _check_bippr(engine, oracle, g, srcs, alpha, rmax_scale=1.0, batch=0, k=0, cap=None, chunk=0):
    """One fora_hip_bippr_batch call (the graph is loaded): every estimate, its sum, the f64 row, the top-k and the
    backward counters equal the twin's.  The first two distinct sources take their walks from the CPU oracle."""
    srcs = np.asarray(srcs, dtype=np.int32)
    rmax, omega, W = br.bippr_setting(g.n, g.m, EPS, rmax_scale)
    tw = _pushes(g, rmax, alpha)
    engine.reset_options()
    if cap is not None:
        engine.set_option("bwd_lds_cap", cap)
    engine.set_option("bwd_chunk", chunk)
    engine.set_batch(batch)
    try:
        ppr, fix, ids, sc, st, bwd = engine.bippr(srcs, epsilon=EPS, rmax_scale=rmax_scale, k=k, want_ppr=True)
        B = engine.get_batch()
    finally:
        engine.set_batch(0)
        engine.reset_options()
    got = {key: bwd[key] for key in STAT_KEYS}
    exp = _expected_stats(tw, g.n, cap, chunk)
    assert got == exp, (cap, chunk, got, exp)
    cpu = list(dict.fromkeys(srcs.tolist()))[:2]
    for i, s in enumerate(srcs.tolist()):
        want = _estimate(engine, oracle, g, s, rmax, W, alpha, s in cpu)
        assert st[i]["n_walks"] == W and st[i]["rmax_used"] == rmax and st[i]["dangling_source"] == int(g.deg[s] == 0)
        assert (fix[i] == want).all(), (i, s, int((fix[i] != want).sum()))
        assert st[i]["ppr_sum_fix"] == sum(int(x) for x in want)
        assert (ppr[i] == np.ldexp(fix[i].astype(np.float64), -60)).all()
        if k:
            want_ids, want_sc = br.topk_of(want, k)
            assert (ids[i] == want_ids).all() and (sc[i] == want_sc).all(), (i, s, k)
    return bwd, _even_batch(srcs.size, B)


@functools.lru_cache(maxsize=None)
def _sources(g):
    """130 sources of tiny_dangling: 100 live ones, 12 dangling ones every ninth place from the fourth on, the first
    source again in the third place, and 17 sources of the first batch again at the end."""
    live = pick_sources(g, 100, 601).tolist()
    dang = pick_sources(g, 12, 602, want_dangling=True).tolist()
    assert len(live) == 100 and len(dang) == 12
    base = live[:2] + live[:1] + live[2:]
    for j, d in enumerate(dang):
        base.insert(3 + 9 * j, d)
    base += base[5:22]
    assert len(base) == 130
    return np.array(base, dtype=np.int32)


def test_bippr_widths_and_uneven_batches(engine, oracle, tiny_dangling):
    g = tiny_dangling
    _load(engine, g, 0.2)
    srcs = _sources(g)
    assert (g.deg[srcs[:33]] == 0).sum() == 4 and (g.deg[srcs[64:]] == 0).sum() >= 5 and srcs[0] == srcs[2]
    widest = 0
    for nq in (1, 33, 64, 65, 130):
        for batch in (0, 1, 48):
            _, per = _check_bippr(engine, oracle, g, srcs[:nq], 0.2, batch=batch)
            if batch == 48 and nq == 130:
                assert per == 44 and nq % per != 0   # batches of 44, 44 and 42
            if batch == 0 and nq == 130:
                if per <= 64:  # the automatic batch is small on this graph: ask for 96
                    _, per = _check_bippr(engine, oracle, g, srcs[:nq], 0.2, batch=96)
                widest = per
    assert widest > 64  # the b0 += 64 loop of the combine and a second tile of the transposes along the slot axis


def test_bippr_chunks_and_tiers_under_the_combine(engine, oracle, tiny_dangling):
    g = tiny_dangling
    _load(engine, g, 0.2)
    srcs = _sources(g)[:5]
    for chunk in (7, 501):
        for batch in (0, 2):
            bwd, per = _check_bippr(engine, oracle, g, srcs, 0.2, batch=batch, cap=40, chunk=chunk)
            assert bwd["chunks"] == -(-g.n // chunk) > 1 and 0 < bwd["global_targets"] < g.n
            assert per == (2 if batch else 5)  # one batch, or batches of 2, 2 and 1
    # 70 slots over several chunks: t0 > 0 together with b0 > 0
    bwd, per = _check_bippr(engine, oracle, g, _sources(g)[:70], 0.2, batch=96, cap=40, chunk=501)
    assert per == 70 and bwd["chunks"] == 4


@pytest.mark.parametrize("alpha", [0.05, 0.5])
def test_bippr_other_alphas(engine, oracle, tiny_dangling, alpha):
    g = tiny_dangling
    _load(engine, g, alpha)
    _check_bippr(engine, oracle, g, _sources(g)[:5], alpha, k=50)
    _check_bippr(engine, oracle, g, _sources(g)[:5], alpha, batch=2, cap=40, chunk=501)
    # deeper pushes (rmax_scale 0.05) on a smaller graph
    n = 600
    rng = np.random.Generator(np.random.PCG64(41))
    m = 6 * n
    h = oracle.Graph.from_edges(n, m, rng.integers(0, n, m).astype(np.int32),
                                np.minimum((n * rng.random(m) ** 2).astype(np.int64), n - 1).astype(np.int32))
    _load(engine, h, alpha)
    dang = np.flatnonzero(h.deg == 0)
    srcs = np.array([5, 300, 5, int(dang[0]) if dang.size else 7, 599], dtype=np.int32)
    rmax = br.bippr_setting(h.n, h.m, EPS, 0.05)[0]
    tw = _pushes(h, rmax, alpha)
    assert tw["stats"]["levels"] >= 6 and max(tw["supports"]) > 300  # (3 levels and 437 of 2000 nodes at the default rmax)
    _check_bippr(engine, oracle, h, srcs, alpha, rmax_scale=0.05, k=10)
    bwd, _ = _check_bippr(engine, oracle, h, srcs, alpha, rmax_scale=0.05, batch=2, cap=40, chunk=7)
    assert bwd["chunks"] > 1 and 0 < bwd["global_targets"] < n


def _double_ring(oracle, half=150):
    """Two nodes per place of a directed ring, both pointing at both nodes of the next place, plus three chords.  The
    two nodes of a place have the same in-neighbours, so their pushes carry the same residues everywhere but on
    themselves, and their estimates from a source elsewhere are equal to the last bit."""
    n = 2 * half
    j = np.arange(half)
    src = np.concatenate([2 * j, 2 * j, 2 * j + 1, 2 * j + 1, [0, 90, 200]])
    nxt = 2 * ((j + 1) % half)
    dst = np.concatenate([nxt, nxt + 1, nxt, nxt + 1, [151, 11, 40]])
    return oracle.Graph.from_edges(n, src.size, src.astype(np.int32), dst.astype(np.int32))


def test_bippr_topk_order_and_ties(engine, oracle, tiny_dangling):
    g = tiny_dangling
    _load(engine, g, 0.2)
    srcs = _sources(g)[:5]
    for k in (1, 50, min(1024, g.n)):
        _check_bippr(engine, oracle, g, srcs, 0.2, k=k)
        _check_bippr(engine, oracle, g, srcs, 0.2, k=k, batch=2, cap=40, chunk=7)
    h = _double_ring(oracle)
    srcs = np.array([0, 77, 0, 298], dtype=np.int32)
    rmax, _, W = br.bippr_setting(h.n, h.m, EPS)
    for alpha in (0.2, 0.5):
        _load(engine, h, alpha)
        for k in (1, 50, min(1024, h.n)):
            _check_bippr(engine, oracle, h, srcs, alpha, k=k)
        _check_bippr(engine, oracle, h, srcs, alpha, k=50, batch=1, cap=1, chunk=7)
        # many estimates are exactly equal, also inside the first 50 (from the twin's rows)
        for s in (0, 77):
            want = _estimate(engine, oracle, h, s, rmax, W, alpha, True)
            _, sc = br.topk_of(want, 50)
            nz = want[want > 0]
            assert nz.size - np.unique(nz).size >= 10 and (np.diff(sc[sc > 0]) == 0).sum() >= 5
