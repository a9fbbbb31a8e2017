"""Life cycle of the state that lives with the graph (fora_hip.hip: struct Graph and its parts, Index, BwdBufs,
SparseResult): one set of base results per graph, then every rebuild of that state -- team tables and hub copy after an
option change, quad copies (built by a load under force_wide) and row split, the global tier and the grow-only backward-push buffers, another graph and
back, the index replaced in place -- and after each of them every call returns the bytes of its base."""
import numpy as np
import pytest

import bippr_ref as br
from conftest import pick_sources
from fora_amd import ForaError

pytestmark = pytest.mark.gpu
SEED = 0x464F5241
EPS = 0.5


def _load(engine, g):
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(epsilon=EPS, seed=SEED)
    return engine.get_params()


def _picks(g, seed):
    """5 sources, one of them dangling; 6 targets, among them the node of largest in-degree and a dangling node."""
    live, dang = pick_sources(g, 4, seed), pick_sources(g, 1, seed + 1, want_dangling=True)
    srcs = np.concatenate([live[:2], dang, live[2:]]).astype(np.int32)
    assert srcs.size == 5 and (g.deg[srcs] == 0).sum() == 1
    hub = int(np.bincount(g.col[:int(g.row_ptr[g.n])], minlength=g.n).argmax())
    tdang = pick_sources(g, 1, seed + 2, want_dangling=True)
    pool = pick_sources(g, 8, seed + 3)
    rest = [int(t) for t in pool if t != hub][:4]
    targets = np.array([rest[0], hub, rest[1], int(tdang[0]), rest[2], rest[3]], dtype=np.int32)
    assert np.unique(targets).size == 6 and (g.deg[targets] == 0).sum() >= 1
    return srcs, targets


def _bytes(*arrays):
    return tuple(np.ascontiguousarray(a).tobytes() for a in arrays)


def _indexed(engine, srcs):
    return _bytes(*engine.query_fix(srcs, with_idx=True)[:2])


def _base(engine, g, srcs, targets, with_bippr):
    """The base set of a graph (its index is in place): every result array as bytes."""
    rmax_b = br.bippr_setting(g.n, g.m, EPS)[0]
    out = {"query": _bytes(*engine.query_fix(srcs)[:2]), "query_idx": _indexed(engine, srcs),
           "bwdpush": _bytes(*engine.bwdpush(targets, rmax_b)[:2]),
           "bippr_targets": _bytes(engine.bippr_targets(srcs, targets)[1])}
    row_ptr, ids, vals, fix = engine.query_sparse(srcs, want_fix=True)[:4]
    out["sparse"] = _bytes(row_ptr, ids, vals, fix)
    if with_bippr:
        out["bippr"] = _bytes(engine.bippr(srcs)[1])  # every node a target: the target buffers grow to n
    return out


def _first_base(engine, oracle, g, srcs, targets, with_bippr):
    """Fresh load, default options: the checked results, the index built and kept, the base set."""
    engine.reset_options()
    rmax, omega = _load(engine, g)
    ppr, res, st = engine.query_fix(srcs)
    for i, s in enumerate(srcs):  # as test_query_bit_exact_vs_twin
        want, wres, wst = oracle.twin_query(g, int(s), rmax, omega, seed=SEED)
        assert (res[i] == wres).all()
        assert (ppr[i] == want).all()
        assert st[i]["n_walks"] == wst["n_walks"] and st[i]["n_idx_hit"] == 0
    rmax_b = br.bippr_setting(g.n, g.m, EPS)[0]
    rsv, rres, _ = engine.bwdpush(targets, rmax_b)
    for i, t in enumerate(targets):
        tw = br.twin_bwd_push(g, int(t), rmax_b)
        assert (rsv[i] == tw["reserve"]).all() and (rres[i] == tw["residue"]).all(), int(t)
    engine.build_index()
    index = engine.get_index()
    base = _base(engine, g, srcs, targets, with_bippr)
    assert base["query"] == _bytes(ppr, res) and base["bwdpush"] == _bytes(rsv, rres)
    return base, index


def _same(engine, g, srcs, targets, base, leg):
    got = _base(engine, g, srcs, targets, "bippr" in base)
    for name in base:
        assert got[name] == base[name], (leg, name)


def _leg_global_tier(engine, g, srcs, targets, base, leg):
    """c: every target on the global tier; then one and four targets per chunk (several chunks, the entry buffers
    regrown and rewritten per batch)."""
    rmax_b = br.bippr_setting(g.n, g.m, EPS)[0]
    engine.set_option("bwd_lds_cap", 0)
    _same(engine, g, srcs, targets, base, leg + " cap 0")
    assert engine.bwdpush(targets, rmax_b)[2]["global_targets"] == targets.size
    for chunk in (1, 4):
        engine.set_option("bwd_chunk", chunk)
        _same(engine, g, srcs, targets, base, "%s chunk %d" % (leg, chunk))
        assert engine.bwdpush(targets, rmax_b)[2]["chunks"] == (targets.size + chunk - 1) // chunk
    engine.reset_options()


def test_results_survive_every_rebuild(engine, oracle, small_dangling, tiny_dangling):
    g, h = small_dangling, tiny_dangling
    srcs, targets = _picks(g, 511)
    hsrcs, htargets = _picks(h, 521)
    try:
        engine.clear_index()
        base, index = _first_base(engine, oracle, g, srcs, targets, False)
        assert engine.get_option("team_members") != 0

        # a: team tables and hub copy follow the options
        engine.set_option("team", 0)
        _same(engine, g, srcs, targets, base, "a team 0")
        assert engine.get_option("team_members") == 0
        engine.set_option("team", -1)
        _same(engine, g, srcs, targets, base, "a team default")
        assert engine.get_option("team_members") != 0
        for size in (2, 4):
            engine.set_option("team_size", size)
            _same(engine, g, srcs, targets, base, "a team_size %d" % size)
            assert engine.get_option("team_members") >= size
        engine.reset_options()

        # b: layout rebuilds.  The option alone re-plans the workspace: wide layout, single-edge reads, the narrow hub copy
        # out of use.  set_graph builds the hub and quad copies for the options in force, so the graph is loaded again
        # under force_wide: quad copies and the hub copy of the wide shift in use.  pass_bins 1: two passes per level, the
        # row split built and the quads out of use; no_split: the row split dropped; then the defaults, loaded afresh
        engine.set_option("force_wide", 1)
        _same(engine, g, srcs, targets, base, "b wide, no quads")
        _load(engine, g)
        engine.set_index(*index)
        _same(engine, g, srcs, targets, base, "b wide, quads")
        engine.set_option("pass_bins", 1)
        _same(engine, g, srcs, targets, base, "b wide, split")
        engine.set_option("no_split", 1)
        _same(engine, g, srcs, targets, base, "b wide, no split")
        engine.reset_options()
        _load(engine, g)
        engine.set_index(*index)
        _same(engine, g, srcs, targets, base, "b defaults")
        assert engine.get_option("team_members") != 0

        # c: global tier and entry buffers
        _leg_global_tier(engine, g, srcs, targets, base, "c small")

        # d: another graph and back.  bippr grows the target buffers to n of the tiny graph, the 6-target calls after it
        # reuse them; the global tier is sized by n and rebuilt for each graph
        hbase, _ = _first_base(engine, oracle, h, hsrcs, htargets, True)
        _same(engine, h, hsrcs, htargets, hbase, "d tiny")
        _leg_global_tier(engine, h, hsrcs, htargets, hbase, "c tiny")
        _load(engine, g)
        with pytest.raises(ForaError) as e:
            engine.sparse_fetch(ids=np.zeros(1, dtype=np.int32), cap=1)
        assert "no sparse result is held" in str(e.value)
        with pytest.raises(ForaError):
            engine.query_fix(srcs, with_idx=True)
        engine.set_index(*index)
        _same(engine, g, srcs, targets, base, "d back")
        _leg_global_tier(engine, g, srcs, targets, base, "c small again")

        # e: the index replaced in place
        for step in ("build", "build again"):
            engine.build_index()
            assert _indexed(engine, srcs) == base["query_idx"], step
        engine.clear_index()
        with pytest.raises(ForaError):
            engine.query_fix(srcs, with_idx=True)
        engine.set_index(*index)
        assert _indexed(engine, srcs) == base["query_idx"]
        for got, want in zip(engine.get_index(), index):
            assert got.tobytes() == want.tobytes()
        _same(engine, g, srcs, targets, base, "e")
    finally:
        engine.clear_index()
        engine.reset_options()
