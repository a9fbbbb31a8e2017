#!/usr/bin/env python3
"""What sparse rows and sweep cuts of seed sets cost on the GPU and what they buy: --sets sets of k_g seeds
each, drawn with replacement across sets from a pool of --pool nodes (so the sets overlap), uniform weights, threshold
1 / n, through four legs in one process,

  (a) Engine.query_seeds_sparse    the set rows stay in HBM; the thresholded CSR comes back
  (b) the way before it: Engine.query_seeds dense words to the host (ns * n of them), then a numpy threshold; its entries
      are asserted equal to leg (a)'s
  (c) Engine.sweep_seeds           the set rows stay in HBM; per set a (len, best, cut, vol, den, conductance) record comes back
  (d) leg (b), then the vectorised numpy sweep of tools/sweep_bench.py over its rows; its best sizes are asserted equal to
      leg (c)'s

Every leg is warmed up once; then the legs run alternately --reps times and a line carries each leg's median and spread
(min, max) in sets/s: a difference smaller than the spread is not a difference.  The comparisons are (a) against (b) and
(c) against (d), each within one run.  Times are a host clock around calls that end in a stream synchronise; compact /
sort / cut ms and batch_ms are the library's device events.  One JSON line per k_g.

  python tools/seeds_outputs_bench.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sweep_bench import host_best  # noqa: E402


def _spread(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--sets", type=int, default=1000)
    ap.add_argument("--pool", type=int, default=1000)
    ap.add_argument("--kg", type=int, nargs="+", default=[1, 10])
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
    rng = np.random.Generator(np.random.PCG64(20261020))
    pool = rng.choice(np.flatnonzero(deg > 0), size=a.pool, replace=False).astype(np.int32)
    rank = np.full(n, -1, dtype=np.int64)

    for kg in a.kg:
        sets = [rng.choice(pool, size=kg, replace=False).tolist() for _ in range(a.sets)]
        flat = (np.arange(a.sets + 1, dtype=np.int64) * kg, np.array(sets, dtype=np.int32).reshape(-1))
        info = {}

        def dense_thresholded():
            out = eng.query_seeds(flat, want_fix=True)
            fix = out["fix"]
            info["dense_bytes"] = fix.nbytes
            thr = np.uint64(info["a"]["sparse"]["thr_fix"])
            rows, ids = np.nonzero(fix >= thr)
            rp = np.zeros(a.sets + 1, dtype=np.int64)
            np.cumsum(np.bincount(rows, minlength=a.sets), out=rp[1:])
            return rp, ids.astype(np.int32), fix[rows, ids]

        def leg_a():
            info["a"] = eng.query_seeds_sparse(flat, want_fix=True)

        def leg_b():
            info["b"] = dense_thresholded()

        def leg_c():
            info["c"] = eng.sweep_seeds(flat)

        def leg_d():
            rp, ids, fix = dense_thresholded()
            info["d_best"] = np.array([host_best(ids[rp[i]:rp[i + 1]], fix[rp[i]:rp[i + 1]], row_ptr, col, deg, nnz, rank)
                                       for i in range(a.sets)], dtype=np.int64)

        legs = [("seeds_sparse", leg_a), ("dense_host_threshold", leg_b), ("seeds_sweep", leg_c), ("dense_host_sweep", leg_d)]

        def agree():
            rp, ids, fix = info["b"]
            assert np.array_equal(rp, info["a"]["row_ptr"]) and np.array_equal(ids, info["a"]["ids"]) and \
                np.array_equal(fix, info["a"]["fix"]), "the host threshold and Engine.query_seeds_sparse disagree on an entry"
            assert (info["d_best"] == info["c"]["rows"]["best"]).all(), "the host sweep and Engine.sweep_seeds disagree on a best size"

        for _, f in legs:
            f()
        agree()
        rate = {name: [] for name, _ in legs}
        stage = {"seeds_sparse": {"compact_ms": [], "batch_ms": []},
                 "seeds_sweep": {"compact_ms": [], "sort_ms": [], "cut_ms": [], "batch_ms": []}}
        for _ in range(a.reps):
            for name, f in legs:
                eng.reset_timing()
                t0 = time.perf_counter()
                f()
                rate[name].append(a.sets / (time.perf_counter() - t0))
                if name in stage:
                    st = info["a"]["sparse"] if name == "seeds_sparse" else info["c"]["sweep"]
                    for k in stage[name]:
                        stage[name][k].append(eng.timing()["batch_ms"] if k == "batch_ms" else st[k])
        agree()
        st, sp, sw = info["a"]["stats"], info["a"]["sparse"], info["c"]["sweep"]
        med = {k: statistics.median(v) for k, v in rate.items()}
        ms = {name: {k: statistics.median(v) for k, v in d.items()} for name, d in stage.items()}
        out = {
            "tool": "seeds_outputs_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "sets": a.sets, "k_g": kg, "pool": a.pool,
            "reps": a.reps, "threshold": 1.0 / n, "seeds": int(st["seeds"]), "distinct": int(st["distinct"]), "queries": int(st["queries"]),
            "batches": int(st["batches"]), "entries": int(sp["entries"]), "max_row": int(sp["max_row"]), "chunks": int(sp["batches"]),
            "sweep_edges": int(sw["edges"]), "global_rows": int(sw["global_rows"]),
            "best_median": int(np.median(info["c"]["rows"]["best"])),
            "conductance_median": round(float(np.median(info["c"]["rows"]["conductance"])), 4),
            "sets_per_s": {k: _spread(v) for k, v in rate.items()},
            "ratio": {"a_over_b": round(med["seeds_sparse"] / med["dense_host_threshold"], 2),
                      "c_over_d": round(med["seeds_sweep"] / med["dense_host_sweep"], 2),
                      "c_over_a": round(med["seeds_sweep"] / med["seeds_sparse"], 3)},
            "stage_ms": {name: {k: _spread(v, 3) for k, v in d.items()} for name, d in stage.items()},
            "share_of_batch_ms": {name: {k: round(d[k] / d["batch_ms"], 4) for k in d if k != "batch_ms"} for name, d in ms.items()},
            "dense_host_bytes": int(info["dense_bytes"]), "sparse_host_bytes": int(sp["entries"]) * 20 + 8 * (a.sets + 1),
        }
        print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
