#!/usr/bin/env python3
"""What local clustering costs on the GPU and what it buys: --sources sources at threshold 1 / n through three
legs in one process,

  (a) Engine.sweep                 the rows stay in HBM; per source a (len, best, cut, vol, den, conductance) record comes back
  (b) today's way: Engine.query_sparse, then a vectorised numpy sweep of the same rows on the host (sort by ppr / degree,
      a rank array, one gather per out-edge of the support, two cumulative sums, the argmin); its best sizes are asserted
      equal to leg (a)'s
  (c) Engine.query_sparse alone    what leg (b) pays before its sweep starts

Every leg is warmed up once; then the legs run alternately --reps times and the line carries each leg's median and spread
(min, max) in sources/s: a difference smaller than the spread is not a difference.  Times are a host clock around calls that
end in a stream synchronise; compact / sort / cut ms and batch_ms are the library's device events.  One JSON line.

  python tools/sweep_bench.py
"""
import argparse
import json
import os
import statistics
import sys
import time
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def host_best(ids, fix, row_ptr, col, deg, nnz, rank):
    """size of the best prefix of one sparse row (ids ascending, fix its words); rank: an all -1 int64 scratch of n entries"""
    if ids.size == 0:
        return 0
    d = deg[ids]
    key = fix // np.maximum(d, 1).astype(np.uint64)
    o = np.lexsort((ids, ~key))
    order, d = ids[o], d[o]
    L = order.size
    rank[order] = np.arange(L)
    first = row_ptr[order]
    pos = np.repeat(np.arange(L), d)
    start = np.cumsum(d) - d
    e = np.repeat(first - start, d) + np.arange(pos.size)
    r = rank[col[e]]
    later = r > pos
    diff = np.bincount(pos[(r < 0) | later], minlength=L) - np.bincount(r[later], minlength=L)
    rank[order] = -1
    cut, vol = np.cumsum(diff), np.cumsum(d)
    den = np.minimum(vol, nnz - vol)
    ok = den > 0
    if not ok.any():
        return 0
    ratio = np.where(ok, cut / np.maximum(den, 1), np.inf)
    cand = np.flatnonzero(ratio <= ratio.min() * (1 + 1e-12))
    return int(min(cand, key=lambda j: (Fraction(int(cut[j]), int(den[j])), j))) + 1


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--sources", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--epsilon", type=float, default=0.5)
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")

    import fora_amd
    from fora_amd import synth
    n, m, row_ptr, col = synth.preset(a.graph)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col)
    deg = np.diff(row_ptr)
    nnz = int(row_ptr[-1])
    eng = fora_amd.Engine(0)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    rng = np.random.Generator(np.random.PCG64(20261019))
    srcs = rng.choice(np.flatnonzero(deg > 0), size=a.sources, replace=False).astype(np.int32)
    rank = np.full(n, -1, dtype=np.int64)
    info = {}

    def leg_a():
        info["a"] = eng.sweep(srcs)

    def leg_b():
        rp, ids, _, fix, _, _ = eng.query_sparse(srcs, want_fix=True)
        info["b_best"] = np.array([host_best(ids[rp[i]:rp[i + 1]], fix[rp[i]:rp[i + 1]], row_ptr, col, deg, nnz, rank)
                                   for i in range(srcs.size)], dtype=np.int64)

    def leg_c():
        info["c"] = eng.query_sparse(srcs, want_fix=True)[-1]

    legs = [("sweep", leg_a), ("sparse_plus_host_sweep", leg_b), ("sparse_only", leg_c)]
    for _, f in legs:
        f()
    assert (info["b_best"] == info["a"]["rows"]["best"]).all(), "the host sweep and Engine.sweep disagree on a best size"
    rate = {name: [] for name, _ in legs}
    stage = {"compact_ms": [], "sort_ms": [], "cut_ms": [], "batch_ms": []}
    for _ in range(a.reps):
        for name, f in legs:
            eng.reset_timing()
            t0 = time.perf_counter()
            f()
            rate[name].append(srcs.size / (time.perf_counter() - t0))
            if name == "sweep":
                for k in ("compact_ms", "sort_ms", "cut_ms"):
                    stage[k].append(info["a"]["sweep"][k])
                stage["batch_ms"].append(eng.timing()["batch_ms"])
    assert (info["b_best"] == info["a"]["rows"]["best"]).all()
    sw = info["a"]["sweep"]
    med = {k: statistics.median(v) for k, v in rate.items()}
    ms = {k: statistics.median(v) for k, v in stage.items()}
    out = {
        "tool": "sweep_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "sources": int(srcs.size), "reps": a.reps,
        "threshold": 1.0 / n, "entries": int(sw["entries"]), "max_row": int(sw["max_row"]), "edges": int(sw["edges"]),
        "batches": int(sw["batches"]), "global_rows": int(sw["global_rows"]),
        "best_median": int(np.median(info["a"]["rows"]["best"])), "conductance_median": round(float(np.median(info["a"]["rows"]["conductance"])), 4),
        "sources_per_s": {k: _spread(v) for k, v in rate.items()},
        "ratio": {"a_over_b": round(med["sweep"] / med["sparse_plus_host_sweep"], 2), "a_over_c": round(med["sweep"] / med["sparse_only"], 3)},
        "stage_ms": {k: _spread(v, 3) for k, v in stage.items()},
        "share_of_batch_ms": {k: round(ms[k] / ms["batch_ms"], 4) for k in ("compact_ms", "sort_ms", "cut_ms")},
        "edges_per_s": round(sw["edges"] / (ms["cut_ms"] * 1e-3)) if ms["cut_ms"] > 0 else None,
    }
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
