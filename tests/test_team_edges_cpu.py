"""The preconditions of tests/test_team_edges_gpu.py, asserted without a GPU: every crafted graph of
tests/team_edge_graphs.py is built, pushed by the CPU twin and laid out by make_team_layout (through tests/tables_check.cpp),
and what the GPU test relies on -- which rows pop in which level, that a threshold ties in its high word, how many heavy rows
one member pops, how many members and local ids the layout has -- is checked here from those two alone."""
import numpy as np
import pytest

import team_edge_graphs as G
from test_tables_cpu import tables_check  # noqa: F401  (the fixture: tests/tables_check.cpp built with the sanitizers)


def _layout(tables_check, tmp_path, g, force, hubs):  # noqa: F811
    f = G.team_layout(tables_check, tmp_path, g, force=force, team_hubs=hubs)
    assert f["team_T"] != 0  # a layout the 24-bit bucket count or the member limit rejects would push without the team
    return f


def test_degree_ladder(oracle, tables_check, tmp_path):  # noqa: F811
    g, f = G.degree_ladder()
    assert g.n == 71027 and g.col.size == 340930
    assert [int(g.deg[h]) for h in f["hubs"]] == list(G.LADDER_DEGREES) and int(g.deg[f["S"]]) == 10
    assert len({h >> 6 for h in f["hubs"]}) == len(f["hubs"])  # ten different 64-node blocks
    indeg = np.bincount(g.col, minlength=g.n)
    assert indeg[f["leaf_back"]] >= 2 and g.deg[f["leaf_back"]] == 1 and g.col[g.row_ptr[f["leaf_back"]]] == f["S"]
    t = G.twin(g, f["S"], 1e-6)
    assert t["levels"] == 20 and t["pops"] == 142878 and t["level_sizes"][:3].tolist() == [1, 10, 70001]
    assert t["level_sizes"][1] == 10 and sorted(G.level1(g, f["S"], 1e-6).tolist()) == f["hubs"]  # all ten hubs pop in level 1
    assert G.twin(g, f["hub_of"][70001], 1e-6)["levels"] == 14
    for d in (8191, 65535):  # as sources: popped in level 0, and their leaves' mass comes back through S
        assert G.twin(g, f["hub_of"][d], 1e-6)["level_sizes"][:2].tolist() == [1, d]
    for force in (0, 16, 32):
        lay = _layout(tables_check, tmp_path, g, force, 1024)
        assert lay["team_T"] == max(8, force) and lay["team_H"] == 1024  # 70 013 nodes with in-edges: eight members at least


TIE_D = (65535, 65536, 70001)


@pytest.mark.parametrize("D", TIE_D)
def test_threshold_tie(oracle, tables_check, tmp_path, D):  # noqa: F811
    g, f = G.threshold_tie(D)
    assert g.n == D + 5 and (g.deg > 0).all() and g.deg[f["H"]] == D  # no node is dangling
    assert f["r_H"] == 0x1999999999999980
    stays, pops = f["cases"]["stays"], f["cases"]["pops"]
    for c in (stays, pops):
        assert c["exact"] and c["high_words_tie"]
    assert not stays["pops_H"] and pops["pops_H"]
    if D > 65535:
        assert stays["saturated_would_pop"]  # a sweep that compared with the saturated degree would pop H
    ts, tp = G.twin(g, f["S"], stays["rmax"]), G.twin(g, f["S"], pops["rmax"])
    assert (ts["levels"], ts["pops"], ts["relax"], int(ts["level_sizes"][1])) == (51, 51, 52, 1)
    assert int(ts["residue"][f["H"]]) == f["r_H"]
    assert (tp["pops"], tp["relax"], int(tp["level_sizes"][1])) == (52, 52 + D, 2)
    assert int(tp["residue"][f["H"]]) != f["r_H"]
    for force in (0, 32):
        assert _layout(tables_check, tmp_path, g, force, 1024)["team_T"] == max(8, force)  # (D + 3 nodes with in-edges)


def test_threshold_equal(oracle, tables_check, tmp_path):  # noqa: F811
    """exact_tie_search (D in 65536 .. 70001, a source of 2 .. 8 out-edges) finds one degree that divides r_H: 69088, for a
    source of 2, 3, 4, 6 or 8 out-edges.  There t1 * D == r_H exactly: `>=` pops the row, `>` would not."""
    found = G.exact_tie_search()
    assert (G.EQUAL_D, 2) in found and {D for D, _ in found} == {G.EQUAL_D}
    g, f = G.threshold_tie(G.EQUAL_D)
    c = f["cases"]["pops"]
    assert c["equal"] and c["exact"] and c["high_words_tie"] and c["pops_H"]
    t = G.twin(g, f["S"], c["rmax"])
    assert (t["pops"], t["relax"], int(t["level_sizes"][1])) == (52, 52 + G.EQUAL_D, 2)
    for force in (0, 32):
        assert _layout(tables_check, tmp_path, g, force, 1024)["team_T"] == max(8, force)  # (D + 3 nodes with in-edges)


@pytest.mark.parametrize("K,T", G.HEAVY_CASES)
def test_many_heavy_rows(oracle, tables_check, tmp_path, K, T):  # noqa: F811
    g, f = G.many_heavy_rows(K, T)
    assert {(h >> 6) % T for h in f["hubs"]} == {0}  # one member owns every hub
    assert [int(g.deg[h]) for h in f["hubs"]] == [G.TEAM_HEAVY + 1 + j for j in range(K)]
    per_member = G.heavy_pops_level1(g, f["S"], 4e-6, T)
    assert per_member.tolist() == [K] + [0] * (T - 1)
    assert (G.TEAM_HEAVY, G.TEAM_NHEAVY) == (1024, 128)  # read from fora_team.h: the cases below are chosen for these two
    assert (K > G.TEAM_NHEAVY) == (K in (129, 160))  # 128 fills the heavy-row table, 129 and 160 overflow it
    t = G.twin(g, f["S"], 4e-6)
    assert t["levels"] == 4 and t["level_sizes"].tolist() == [1, K, 1300, 1]
    if (K, T) == (160, 1):
        assert g.col.size == 177530 and int((np.bincount(g.col, minlength=g.n) > 0).sum()) == 1461
        deep = G.twin(g, f["S"], 1e-7)
        assert deep["levels"] == 19 and deep["level_sizes"][:6].tolist() == [1, 160, 1300, 1, 160, 1300]  # the hubs pop again in level 4
    for hubs in (0, 1024):
        lay = _layout(tables_check, tmp_path, g, T, hubs)
        assert lay["team_T"] == T and lay["team_H"] == hubs


def test_spare_source(oracle, tables_check, tmp_path):  # noqa: F811
    g, f = G.spare_source()
    assert g.n == 200 and np.bincount(g.col, minlength=g.n)[f["S"]] == 0 and g.deg[8] == 0 and g.deg[6] == 1
    t = G.twin(g, f["S"], 1e-3)
    assert t["levels"] == 24 and t["pops"] == 105 and t["level_sizes"][:4].tolist() == [1, 6, 2, 7]
    assert G.twin(g, f["S"], 1e-9)["levels"] == 86
    # the source pops again and again: its reserve is more than the alpha of its first pop
    assert int(t["reserve"][f["S"]]) > int(G.FIX_ONE * G.ALPHA) + 1 and int(t["residue"][f["S"]]) > 0
    lay = _layout(tables_check, tmp_path, g, 0, 1024)
    assert lay["team_T"] == 1 and lay["team_R"] == 64 and lay["team_H"] == 200


@pytest.mark.parametrize("hubs", [0, 1, 2048, 4096])
def test_hub_counts_on_the_session_graph(oracle, tables_check, tmp_path, small_dangling, hubs):  # noqa: F811
    lay = _layout(tables_check, tmp_path, small_dangling, 0, hubs)
    assert lay["team_H"] == hubs  # (not cut: the graph's residues leave room for 4096 sums)


def test_ids_at_cap(oracle, tables_check, tmp_path):  # noqa: F811
    cap = G.team_r_cap(tables_check, tmp_path)
    assert cap % 64 == 0 and cap > 4096
    for extra, T in ((0, 1), (1, 2)):
        g, f = G.ids_at_cap(cap, extra)
        assert g.n == cap + extra and np.bincount(g.col, minlength=g.n).min() >= 1  # every node takes a local id
        assert len(f["sources"]) == 5 and (g.deg[f["sources"]] > 0).all()
        for hubs in (1024, 4096):
            lay = _layout(tables_check, tmp_path, g, 0, hubs)
            assert lay["team_T"] == T and lay["team_R_cap"] == cap
            assert lay["team_R"] == cap if extra == 0 else 64 <= lay["team_R"] < cap
            if (extra, hubs) == (0, 4096):
                assert 1024 < lay["team_H"] < 4096 and lay["team_H"] < g.n  # cut by the LDS the residues leave
                assert lay["team_H"] == 2239  # as the checker reports it today (DESIGN.md 5.1 quotes it): 160 KiB - 23 KiB - 8 * (R + 1), in 8-byte sums
            else:
                assert lay["team_H"] == hubs
