"""What the tests of the seed sets' sparse rows and sweeps share (test_seeds_outputs_cpu.py, test_seeds_sparse_gpu.py,
test_seeds_sweep_gpu.py): the sets of one call, the expected set rows -- single-seed rows folded by seeds_ref.combine in Python
ints, never through the code under test -- their thresholded CSR, and the node a threshold after the sum keeps where a merge
of per-seed thresholded rows loses it."""
import math

import numpy as np

import seeds_ref as sr

SEED = 0x464F5241
ALPHA = 0.2
EPS = 0.5
ONE = 1 << 62


def thr_fix_of(t):
    return 1 if t <= 0 else max(1, math.ceil(math.ldexp(t, 62)))


def pick(g, count, seed, want_dangling=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    pool = np.flatnonzero(g.deg == 0) if want_dangling else np.flatnonzero(g.deg > 0)
    if pool.size == 0:
        return []
    return [int(x) for x in rng.choice(pool, size=min(count, pool.size), replace=False)]


def sets_of(g):
    """The sets of one call and a weight list of the same shape: a singleton, 3 seeds, a duplicate seed plus a dangling one,
    (where the graph has dangling nodes) dangling seeds only, two overlapping sets, a duplicate set, 11 seeds over three
    batches at set_batch(4)."""
    live = pick(g, 16, 601)
    dang = pick(g, 2, 602, want_dangling=True)
    sets = [
        [live[0]],
        [live[1], live[2], live[3]],
        [live[4], live[5], live[4]] + dang[:1],
        [live[0], live[1], live[2], live[3], live[14]],
        [live[0], live[1], live[2], live[3], live[15]],
        [live[1], live[2], live[3]],
        live[3:14],
    ]
    if dang:
        sets.insert(3, [dang[0], dang[-1], dang[0]])
    rng = np.random.Generator(np.random.PCG64(603))
    weights = [[float(x) for x in rng.integers(1, 1000, size=len(s)) / 64.0] for s in sets]
    weights[0] = [0.3]
    weights[2] = [0.5, 1.25, 2.0, 0.75][:len(sets[2])]
    weights[-1][4] = 0.0
    return sets, weights


def load(engine, g):
    engine.clear_index()
    engine.reset_options()
    engine.set_batch(0)
    engine.set_balanced(False)
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(alpha=ALPHA, epsilon=EPS, seed=SEED)


class Case:
    """sets, weights, rows (seed -> its query_fix row as ints), and per weighting ("u" uniform, "w" weighted) the wfix lists
    and the expected set rows"""


_REF = {}


def reference(engine, g, with_idx=False):
    """Per graph, once.  The engine must be loaded with g (and hold its index for with_idx)."""
    key = (id(g), with_idx)
    if key not in _REF:
        c = Case()
        c.g = g
        c.sets, c.weights = sets_of(g)
        distinct = sorted({s for st in c.sets for s in st})
        fix, _, _ = engine.query_fix(np.array(distinct, dtype=np.int32), with_idx=with_idx, want_residue=False)
        c.rows = {s: fix[i].tolist() for i, s in enumerate(distinct)}
        for s in distinct:
            if g.deg[s] == 0:
                assert c.rows[s][s] == ONE and sum(c.rows[s]) == ONE
        c.wfix = {"u": [sr.uniform_wfix(len(st)) for st in c.sets], "w": [sr.weighted_wfix(w) for w in c.weights]}
        c.expect = {k: [sr.combine([c.rows[s] for s in st], w) for st, w in zip(c.sets, c.wfix[k])] for k in ("u", "w")}
        _REF[key] = c
    return _REF[key]


def counts(g, sets, dedup=1):
    listed = [s for st in sets for s in st]
    live = [s for s in listed if g.deg[s] > 0]
    return dict(seeds=len(listed), distinct=len(set(listed)), dangling=len(listed) - len(live),
                queries=len(set(live)) if dedup else len(live))


def csr_of(rows, thr):
    """(row_ptr, ids, fix) of the rows thresholded at thr units: ids ascending inside a row, words unchanged"""
    row_ptr, ids, fix = [0], [], []
    for row in rows:
        for v, x in enumerate(row):
            if x >= thr:
                ids.append(v)
                fix.append(x)
        row_ptr.append(len(ids))
    return row_ptr, ids, fix


def lifted_node(seed_rows, wfix):
    """A node the sum lifts over a threshold that each of its terms misses.  seed_rows: the single-seed rows of one set, wfix
    their weights.  Returns (v, thr, terms): thr = row[v] of the combined row for a v with two or more non-zero terms
    floor(wfix_j * x_j[v] / 2^62) -- every term is then under thr -- taken among the v whose word is below 2^53, so that
    thr * 2^-62 is a double and a call can ask for exactly this threshold; the largest such word, ties to the smaller id.
    None when the set has no such node."""
    best = None
    for v in range(len(seed_rows[0])):
        terms = [(w * int(x[v])) >> 62 for x, w in zip(seed_rows, wfix)]
        total = sum(terms)
        if sum(1 for t in terms if t) >= 2 and total < 1 << 53 and (best is None or total > best[1]):
            best = (v, total, terms)
    return best


def merge_thresholded(seed_rows, wfix, thr):
    """What a host gets without the feature: every seed's weighted row thresholded on its own, the kept entries merged.
    Returns {v: sum of the kept terms}."""
    out = {}
    for x, w in zip(seed_rows, wfix):
        for v, xv in enumerate(x):
            t = (w * int(xv)) >> 62
            if t >= thr:
                out[v] = out.get(v, 0) + t
    return out
