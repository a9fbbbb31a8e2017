"""Crafted graphs for the edges of k_push_team (fora_amd/csrc/fora_team.h) and the facts about them that the tests assert.

Plain numpy and the CPU twin (oracle/fora_twin.c through oracle_lib): no GPU, no torch.  Every builder returns an
oracle_lib.Graph and a dict of facts; tests/test_team_edges_cpu.py asserts the facts from the twin and the host-side table
builder alone, tests/test_team_edges_gpu.py runs the team push on the same graphs.

  degree_ladder     rows of 1023 ... 70001 edges: the heavy-row bound (1024 / 1025), the 13-bit degree of a pop (8191 in
                    TeamDev::rowl: look it up), the 16-bit degree of the sweep (0xFFFF in TeamDev::deg16: look it up)
  threshold_tie     one row of D >= 65535 edges whose residue and threshold agree in their high words: the sweep's exact
                    comparison with the looked-up degree decides whether the row pops
  many_heavy_rows   more rows over TEAM_HEAVY edges in one level of one member than the heavy-row table has entries
  spare_source      a source without in-edges that dangling nodes keep handing their mass back to: the spare local id R
  ids_at_cap        exactly TEAM_R_CAP nodes with in-edges (one member, the tightest LDS fit), and one more (two members)
"""
import functools

import numpy as np

import oracle_lib as orc

ALPHA = 0.2
FIX_ONE = orc.FIX_ONE


def _team_define(name):
    """The default of a `#define` of fora_team.h, read from the header: the builders follow the kernel's numbers."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fora_amd", "csrc", "fora_team.h")
    with open(path) as f:
        found = re.findall(rf"^#define {name} (\d+)\b", f.read(), flags=re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


TEAM_HEAVY = _team_define("FORA_TEAM_HEAVY")    # a popped row of more edges is shared out through the heavy-row table ...
TEAM_NHEAVY = _team_define("FORA_TEAM_NHEAVY")  # ... which has this many entries per member and level


def _graph(n, src, dst):
    src = np.concatenate([np.asarray(s, dtype=np.int32).ravel() for s in src])
    dst = np.concatenate([np.asarray(d, dtype=np.int32).ravel() for d in dst])
    return orc.Graph.from_edges(int(n), int(src.size), src, dst)


def t1_of(rmax):
    """The threshold unit of the twin and the engine: ceil(rmax * 2^62)."""
    return int(orc.lib().orc_twin_rmax_fix(orc._d(rmax)))


def node_thr(t1, deg):
    return 1 if deg == 0 else min(t1 * int(deg), (1 << 64) - 1)


_TWIN = {}


def twin(g, s, rmax):
    """oracle_lib.twin_push, computed once per (graph, source, rmax) and shared: the arrays are never written to."""
    key = (id(g), int(s), float(rmax))
    if key not in _TWIN:
        t = orc.twin_push(g, int(s), rmax, alpha=ALPHA)
        t["residue"].setflags(write=False)
        t["reserve"].setflags(write=False)
        _TWIN[key] = (g, t)  # (holds g: its id stays taken)
    return _TWIN[key][1]


def level1(g, s, rmax):
    """The nodes popped in level 1: the out-neighbours of s that the source's pop lifts to their threshold (a node named
    twice by the row gets two increments)."""
    t1 = t1_of(rmax)
    deg = g.deg
    row = g.col[g.row_ptr[s]:g.row_ptr[s + 1]]
    afix = int(orc.lib().orc_twin_alpha_fix(orc._d(ALPHA)))
    keep = (FIX_ONE * afix) >> 62
    inc = (FIX_ONE - keep) // int(deg[s])
    tg, cnt = np.unique(row, return_counts=True)
    return np.array([v for v, c in zip(tg, cnt) if v != s and inc * int(c) >= node_thr(t1, deg[v])], dtype=np.int64)


# ---------------------------------------------------------------- degree ladder
LADDER_DEGREES = (1023, 1024, 1025, 8190, 8191, 8192, 65534, 65535, 65536, 70001)
LADDER_POOL = 70001


@functools.lru_cache(maxsize=None)
def degree_ladder():
    """S = 0 -> ten hubs (ids 64 * (j + 1): ten different 64-node blocks) of LADDER_DEGREES out-edges; hub j names d_j
    distinct leaves of a pool of 70001, from offset 7919 * j (mod the pool).  Of the leaves a third are dangling, a third
    point back to S, a third point to a node M whose one edge ends at a dangling node."""
    S, first_leaf = 0, 1024
    hubs = [64 * (j + 1) for j in range(len(LADDER_DEGREES))]
    M = first_leaf + LADDER_POOL
    E = M + 1
    n = E + 1
    src, dst = [np.full(len(hubs), S)], [np.array(hubs)]
    for j, (h, d) in enumerate(zip(hubs, LADDER_DEGREES)):
        src.append(np.full(d, h))
        dst.append(first_leaf + (7919 * j + np.arange(d)) % LADDER_POOL)
    i = np.arange(LADDER_POOL)
    back, mid = i[i % 3 == 0], i[i % 3 == 1]  # (i % 3 == 2: dangling)
    src += [first_leaf + back, first_leaf + mid, [M]]
    dst += [np.full(back.size, S), np.full(mid.size, M), [E]]
    g = _graph(n, src, dst)
    facts = dict(S=S, hubs=hubs, degrees=LADDER_DEGREES, leaf_back=first_leaf + 3, leaf_dangling=first_leaf + 2, M=M, E=E,
                 hub_of={d: h for h, d in zip(hubs, LADDER_DEGREES)})
    return g, facts


# ---------------------------------------------------------------- threshold tie
@functools.lru_cache(maxsize=None)
def threshold_tie(D, src_deg=2):
    """S -> H and S -> X_1 .. X_(src_deg - 1); H -> D leaves; every leaf -> a; every X -> a; a <-> b.  No node is dangling:
    nothing returns to S.  One twin push at rmax 0.45 pops the source alone and leaves r_H = residue[H]; the thresholds
    are then set around r_H / D: "stays" t1 = r_H // D + 1 (t1 * D > r_H), "pops" t1 = r_H // D (t1 * D <= r_H)."""
    S, H, a, b = 0, 1, 2, 3
    X = list(range(4, 4 + src_deg - 1))
    first_leaf = 4 + src_deg - 1
    leaves = first_leaf + np.arange(D)
    n = first_leaf + D
    g = _graph(n, [[S], np.full(len(X), S), np.full(D, H), leaves, X, [a], [b]],
               [[H], X, leaves, np.full(D, a), np.full(len(X), a), [b], [a]])
    first = orc.twin_push(g, S, 0.45, alpha=ALPHA)
    assert first["pops"] == 1 and first["levels"] == 1
    r_H = int(first["residue"][H])
    cases = {}
    for name, t1 in (("stays", r_H // D + 1), ("pops", r_H // D)):
        rmax = float(np.ldexp(float(t1), -62))
        cases[name] = dict(
            t1=t1, rmax=rmax,
            exact=(t1 < (1 << 53) and t1_of(rmax) == t1),                     # the double carries t1 exactly
            high_words_tie=((t1 * D) >> 32) == (r_H >> 32),                   # the sweep enters its exact comparison
            saturated_would_pop=r_H >= t1 * min(D, 65535),                    # what a sweep on deg16 alone would decide
            pops_H=r_H >= t1 * D,
            equal=t1 * D == r_H)
    return g, dict(S=S, H=H, X=X, a=a, b=b, D=D, r_H=r_H, cases=cases)


EQUAL_D = 69088  # the one degree in 65536 .. 70001 that divides r_H (exact_tie_search; tests/test_team_edges_cpu.py asserts it)


def exact_tie_search():
    """(D, src_deg) with r_H divisible by D, D in 65536 .. 70001 and a source of 2 .. 8 out-edges: there t1 * D == r_H can be
    set exactly, which tells `>=` from `>`.  r_H does not depend on D: it is read from a graph with D = 1."""
    found = []
    for k in range(2, 9):
        _, f = threshold_tie(1, k)
        found += [(D, k) for D in range(65536, 70002) if f["r_H"] % D == 0]
    return found


# ---------------------------------------------------------------- many heavy rows
@functools.lru_cache(maxsize=None)
def many_heavy_rows(K, T):
    """S = 0 -> K hubs; hub j has 1025 + j out-edges into a pool of 1300 leaves (from leaf 37 * j on, mod the pool); every
    second leaf points back to S.  The hub ids are 64 * T * (j + 1): under owner(v) = (v >> 6) % T all of them, and S,
    belong to member 0."""
    S, pool = 0, 1300
    hubs = [64 * T * (j + 1) for j in range(K)]
    first_leaf = 64 * T * (K + 1)
    n = first_leaf + pool
    src, dst = [np.full(K, S)], [np.array(hubs)]
    for j, h in enumerate(hubs):
        d = TEAM_HEAVY + 1 + j
        assert d <= pool
        src.append(np.full(d, h))
        dst.append(first_leaf + (37 * j + np.arange(d)) % pool)
    even = first_leaf + np.arange(0, pool, 2)
    src.append(even)
    dst.append(np.full(even.size, S))
    return _graph(n, src, dst), dict(S=S, hubs=hubs, K=K, T=T, first_leaf=first_leaf)


HEAVY_CASES = ((128, 1), (129, 1), (160, 1), (160, 4))  # (K, T): the table full, one row over, many over, and a team of four


def heavy_pops_level1(g, s, rmax, T):
    """Per member of a team of T: rows over TEAM_HEAVY edges among the nodes popped in level 1."""
    fr = level1(g, s, rmax)
    heavy = fr[g.deg[fr] > TEAM_HEAVY]
    return np.bincount((heavy >> 6) % T, minlength=T)


# ---------------------------------------------------------------- spare source
@functools.lru_cache(maxsize=None)
def spare_source():
    """n = 200: 0 -> 1 .. 5 (dangling) and 0 -> 6 -> 7 -> 8 (dangling).  Node 0 has no in-edge: as a source it uses the spare
    local id, and the dangling nodes hand their mass back to it level after level."""
    n = 200
    g = _graph(n, [np.zeros(6), [6, 7]], [np.arange(1, 7), [7, 8]])
    return g, dict(S=0)


# ---------------------------------------------------------------- ids at the cap
@functools.lru_cache(maxsize=None)
def ids_at_cap(cap, extra):
    """n = cap + extra nodes on a ring v -> v + 1 (every node has an in-edge: every node takes a local id) with three more
    pseudo-random out-edges per node."""
    n = cap + extra
    v = np.arange(n)
    rnd = np.random.Generator(np.random.PCG64(0x1D5A7CA9)).integers(0, n, size=(n, 3))
    g = _graph(n, [v, np.repeat(v, 3)], [(v + 1) % n, rnd])
    return g, dict(sources=[0, 1, n // 2, 7777, n - 1])


# ---------------------------------------------------------------- the host-side layout of a graph (tests/tables_check.cpp)
def team_layout(exe, folder, g, force=0, team_hubs=1024, max_members=32):
    """What make_team_layout (fora_tables.h) decides for g under the options `team_size` = force and `team_hubs`, as the
    stand-alone checker reports it: team_T (0: no team push), team_R, team_H and team_R_cap (TEAM_R_CAP of fora_consts.h)."""
    from test_tables_cpu import _run, _write
    path = _write(folder / f"g{id(g)}.csr", g.row_ptr, g.col)
    return _run(exe, path, force=force, max_members=max_members, team_hubs=team_hubs, tables=["team"])


def team_r_cap(exe, folder):
    return team_layout(exe, folder, spare_source()[0])["team_R_cap"]
