"""k_push_team (fora_amd/csrc/fora_team.h) held to the CPU twin on the crafted graphs of tests/team_edge_graphs.py: the
degree look-ups of a pop (13 bits) and of the sweep (16 bits), a threshold that ties in its high word, more heavy rows than
the heavy-row table holds, hub sums beyond one per thread, the spare local id of a source without in-edges, and a member
with exactly TEAM_R_CAP local ids.  tests/test_team_edges_cpu.py asserts, without a GPU, that the graphs reach those paths.

Every comparison is an equality of bits and counters with oracle/fora_twin.c.  A team launch that times out is run again
through the bucketed kernels and returns the right bits, so every team run here also asserts that the team kernel was
launched, that the bucketed kernels were not, and that no fallback was counted.  Every case runs once more with the
bucketed kernels (team = 0, tail = 0) against the same twin results: a failure of the team run alone belongs to k_push_team.
"""
import os
import subprocess

import numpy as np
import pytest

import team_edge_graphs as G
from conftest import pick_sources

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x464F5241
OMEGA = 1000.0  # only push() is called: no walk is drawn


@pytest.fixture(scope="module")
def tables_check(tmp_path_factory):
    """tests/tables_check.cpp built plainly: here it only reports the layout (team_R_cap, team_T, team_R, team_H).  The build
    with the sanitizers belongs to the CPU tests (tests/test_tables_cpu.py, tests/test_team_edges_cpu.py)."""
    exe = str(tmp_path_factory.mktemp("tables_plain") / "tables_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "tables_check.cpp")], check=True)
    return exe


def _same_as_twin(g, srcs, rmax, rsv, res, st, what):
    for i, s in enumerate(srcs):
        t = G.twin(g, int(s), rmax)
        got = (int(st[i]["pops"]), int(st[i]["relax"]), int(st[i]["levels"]))
        assert got == (t["pops"], t["relax"], t["levels"]), f"{what}: slot {i} (source {s}): (pops, relax, levels) {got}, twin {(t['pops'], t['relax'], t['levels'])}"
        for name, a, b in (("residue", res[i], t["residue"]), ("reserve", rsv[i], t["reserve"])):
            bad = np.flatnonzero(a != b)
            assert bad.size == 0, f"{what}: slot {i} (source {s}): {name} differs at {bad.size} nodes, first {bad[0]}: {int(a[bad[0]]):#x}, twin {int(b[bad[0]]):#x}"
        assert int(st[i]["rsum_fix"]) == t["rsum_fix"], f"{what}: slot {i} (source {s}): rsum_fix"


def _load(engine, g, rmax, opts):
    engine.clear_index()
    for k, v in opts.items():
        engine.set_option(k, v)  # before set_graph: team_size and team_hubs are read when the tables are built
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    if rmax is None:
        engine.set_params(epsilon=0.5, seed=SEED)
        rmax = engine.get_params()[0]
    else:
        engine.set_params_raw(0.2, rmax, OMEGA, seed=SEED)
    return rmax


def _team_push(engine, g, srcs, rmax, **opts):
    """One push of srcs through k_push_team (rmax None: epsilon 0.5 through set_params), bit for bit the twin's."""
    srcs = np.asarray(srcs, dtype=np.int32)
    rmax = _load(engine, g, rmax, dict(team=1, **opts))
    fb0 = engine.get_option("team_fallbacks")
    engine.reset_timing()
    rsv, res, st = engine.push(srcs)
    tm = engine.timing()
    what = f"team push {opts}"
    assert tm["push_team_launches"] >= 1, f"{what}: k_push_team was not launched"
    assert tm["push_expand_launches"] == 0, f"{what}: the bucketed kernels ran"
    assert engine.get_option("team_fallbacks") == fb0, f"{what}: the call was run again through the bucketed kernels"
    assert engine.get_option("team_suspended") == 0
    _same_as_twin(g, srcs, rmax, rsv, res, st, what)
    return rsv, res, st


def _bucketed_push(engine, g, srcs, rmax):
    srcs = np.asarray(srcs, dtype=np.int32)
    rmax = _load(engine, g, rmax, dict(team=0, tail=0))
    engine.reset_timing()
    rsv, res, st = engine.push(srcs)
    assert engine.timing()["push_team_launches"] == 0
    _same_as_twin(g, srcs, rmax, rsv, res, st, "bucketed push")


# ---------------------------------------------------------------- 1. degree ladder
def _ladder_sources(f):
    return [f["S"], f["hub_of"][8191], f["hub_of"][65535], f["hub_of"][70001], f["leaf_back"], f["S"]]


@pytest.mark.parametrize("opts", [dict(team_size=0, team_log=-1),
                                  dict(team_size=32, team_log=0, team_tail=0, tail=0),
                                  dict(team_size=16, team_log=7, team_tail=300, tail_always=1),
                                  dict(team_max=1)],
                         ids=["fewest-members", "size32-nolog-notail", "size16-log7-tail300", "one-team"])
def test_degree_ladder(engine, oracle, opts):
    """Rows of 1023, 1024, 1025 (TEAM_HEAVY), 8190, 8191, 8192 (rowl's 13 bits, fora_team.h:685-686), 65534, 65535, 65536 and
    70001 edges (deg16's 16 bits, :255 and :496-500) popped in one level, and three of them as sources.  team_log 0: every
    pop goes through the accumulator path; team_max 1: one team takes the six slots in turn, and what a slot leaves in
    rsvl, the hub sums and the log must not reach the next one."""
    g, f = G.degree_ladder()
    srcs = _ladder_sources(f)
    try:
        rsv, res, _ = _team_push(engine, g, srcs, 1e-6, **opts)
        assert (rsv[0] == rsv[5]).all() and (res[0] == res[5]).all()  # the repeated source
        if "team_max" in opts:
            _bucketed_push(engine, g, srcs, 1e-6)
    finally:
        engine.reset_options()


# ---------------------------------------------------------------- 2. threshold tie
@pytest.mark.parametrize("size", [0, 32])
@pytest.mark.parametrize("D", [65535, 65536, 70001, G.EQUAL_D])
def test_threshold_tie(engine, oracle, D, size):
    """residue[H] and t1 * D agree in their high 32 bits: the sweep takes its exact comparison (fora_team.h:493-503) with the
    degree it looks up (:496-500).  One unit of t1 decides whether H pops; D = 69088 divides the residue: t1 * D equals it."""
    g, f = G.threshold_tie(D)
    H = f["H"]
    names = ("pops",) if D == G.EQUAL_D else ("stays", "pops")
    try:
        for name in names:
            c = f["cases"][name]
            assert c["exact"] and c["high_words_tie"] and c["pops_H"] == (name == "pops") and c["equal"] == (D == G.EQUAL_D)
            t = G.twin(g, f["S"], c["rmax"])
            rsv, res, st = _team_push(engine, g, [f["S"]], c["rmax"], team_size=size)
            # (already equal to the twin; said again so that a failure names the decision)
            assert int(st[0]["relax"]) == t["relax"] == (52 + D if name == "pops" else 52), f"H {name}: relaxations"
            assert int(res[0][H]) == int(t["residue"][H]) and (int(res[0][H]) == f["r_H"]) == (name == "stays"), f"H {name}: residue[H]"
            if size == 0:
                _bucketed_push(engine, g, [f["S"]], c["rmax"])
    finally:
        engine.reset_options()


# ---------------------------------------------------------------- 3. many heavy rows
@pytest.mark.parametrize("hubs", [0, 1024])
@pytest.mark.parametrize("K,T,rmax", [(K, T, 4e-6) for K, T in G.HEAVY_CASES] + [(160, 1, 1e-7)])
def test_many_heavy_rows(engine, oracle, K, T, rmax, hubs):
    """One member pops K rows of 1025 ... 1184 edges in level 1: 128 fill h_ent / h_deg / h_cstart, the 129th and later stay
    with the wave that popped them -- rows of more than 256 quads through the mark scan and its carry (fora_team.h:700-758).
    team_hubs 0: every edge is a message; 1024: most are hub sums.  rmax 1e-7: the hubs pop in two levels."""
    g, f = G.many_heavy_rows(K, T)
    assert G.heavy_pops_level1(g, f["S"], rmax, T)[0] == K
    try:
        _team_push(engine, g, [f["S"]], rmax, team_size=T, team_hubs=hubs)
        if hubs == 0:
            _bucketed_push(engine, g, [f["S"]], rmax)
    finally:
        engine.reset_options()


# ---------------------------------------------------------------- 4. hub sums
@pytest.mark.parametrize("hubs", [0, 1, 2048, 4096])
def test_hub_sums(engine, oracle, small_dangling, hubs):
    """team_hubs beyond one per thread: the end of a level reads hubtgt[h] for h >= 1024 (fora_team.h:829-839)."""
    g = small_dangling
    srcs = np.concatenate([pick_sources(g, 9, 151), pick_sources(g, 2, 152, want_dangling=True)])
    try:
        _team_push(engine, g, srcs, None, team_hubs=hubs)
        assert engine.get_option("team_hub_sums") == hubs
        if hubs == 0:
            _bucketed_push(engine, g, srcs, None)
    finally:
        engine.reset_options()


# ---------------------------------------------------------------- 5. spare source
@pytest.mark.parametrize("log", [0, -1])
@pytest.mark.parametrize("tail", [dict(team_tail=0, tail=0), dict(team_tail=64, tail_always=1)], ids=["to-the-end", "hand-over"])
@pytest.mark.parametrize("rmax", [1e-3, 1e-9])
def test_spare_source(engine, oracle, rmax, tail, log):
    """A source without in-edges that dangling nodes hand their mass back to: the spare local id R.  Its pops add to
    ppr[src] directly and leave an empty log entry (fora_team.h:680-692); to the end, its residue is written at :579; with
    the hand-over it takes the spare entry of the list (:538-545)."""
    g, f = G.spare_source()
    try:
        _team_push(engine, g, [f["S"]], rmax, team_log=log, **tail)
        _team_push(engine, g, [0, 6, 0, 8], rmax, team_log=log, team_max=1, **tail)  # 6 has an in-edge, 8 is dangling
        if log == -1:
            _bucketed_push(engine, g, [0, 6, 0, 8], rmax)
    finally:
        engine.reset_options()


# ---------------------------------------------------------------- 6. ids at the cap
@pytest.mark.parametrize("hubs", [1024, 4096])
@pytest.mark.parametrize("extra", [0, 1])
def test_ids_at_cap(engine, oracle, tables_check, tmp_path, extra, hubs):
    """TEAM_R_CAP nodes with in-edges: one member, 240 id groups, every sweep iteration in use, and with team_hubs 4096 the
    hub sums cut to the LDS that is left (fora_tables.h:309-310).  One node more: two members."""
    cap = G.team_r_cap(tables_check, tmp_path)
    g, f = G.ids_at_cap(cap, extra)
    lay = G.team_layout(tables_check, tmp_path, g, force=0, team_hubs=hubs)
    assert lay["team_T"] == 1 + extra
    try:
        _team_push(engine, g, f["sources"], None, team_hubs=hubs)
        assert engine.get_option("team_members") == lay["team_T"]
        assert engine.get_option("team_local_ids") == lay["team_R"]
        assert engine.get_option("team_hub_sums") == lay["team_H"]
        if hubs == 1024:
            _bucketed_push(engine, g, f["sources"], None)
            assert engine.get_option("team_members") == 0 and engine.get_option("team_local_ids") == 0 and engine.get_option("team_hub_sums") == 0
    finally:
        engine.reset_options()


# ---------------------------------------------------------------- 7. one whole query on the ladder
def test_query_on_the_ladder(engine, oracle):
    """The whole query from S and from the row of 70001 edges: that row also goes through the degree-grouped walk copy."""
    g, f = G.degree_ladder()
    rmax, omega = 1e-5, 4000.0
    srcs = np.array([f["S"], f["hub_of"][70001]], dtype=np.int32)
    try:
        engine.clear_index()
        engine.set_graph(g.n, g.m, g.row_ptr, g.col)
        engine.set_params_raw(0.2, rmax, omega, seed=SEED)
        fb0 = engine.get_option("team_fallbacks")
        engine.reset_timing()
        ppr, res, st = engine.query_fix(srcs)
        tm = engine.timing()
        assert tm["push_team_launches"] >= 1 and tm["push_expand_launches"] == 0 and engine.get_option("team_fallbacks") == fb0
        assert engine.get_option("team_suspended") == 0
        for i, s in enumerate(srcs):
            want, wres, wst = oracle.twin_query(g, int(s), rmax, omega, seed=SEED)
            assert 1000 <= wst["n_walks"] < 20000  # (the twin draws 19 411 walks from S and 1987 from the hub)
            assert (res[i] == wres).all() and (ppr[i] == want).all()
            assert st[i]["ppr_sum_fix"] == oracle.FIX_ONE and st[i]["n_walks"] == wst["n_walks"]
    finally:
        engine.reset_options()
