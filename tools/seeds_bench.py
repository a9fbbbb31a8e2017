#!/usr/bin/env python3
"""What seed-set queries cost and what they buy: --sets sets of k_g seeds each, drawn with replacement across
sets from a pool of --pool nodes (so the sets overlap), uniform weights, through four legs in one process,

  (a) query_seeds, top-k only                 the set rows stay in HBM, ns * k (ids, scores) come back
  (b) query_seeds, dense rows to the host     ns * n doubles come back
  (c) today's way: Engine.query dense rows of the distinct seeds, then a numpy weighted sum per set on the host, over the
      same sets as every other leg (at k_g = 100 the host sum of 1000 sets moves 225 GB through the CPU: about 35 s).
      --host-sets N runs it on the first N sets only, for a quick look; the ratios of such a line compare unlike
      workloads (the subset has less overlap per set) and the line says so in "like_for_like"
  (d) leg (a) with the option seeds_dedup = 0  every listed seed runs as a query of its own

Every leg is warmed up once; then the legs run alternately --reps times and a line carries each leg's median and spread
(min, max) in sets/s: a difference smaller than the spread is not a difference.  Times are a host clock around calls that
end in a stream synchronise; combine_ms and batch_ms are the library's device events.  One JSON line per k_g.

  python tools/seeds_bench.py
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


def _spread(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def _combine_bytes(sets, slots_of, batch, n):
    """Bytes k_seed_combine moves: 8 n per use, 16 n (read + write of the accumulator row) per (set, batch) touched."""
    nl = len(slots_of)
    per = nl if nl <= batch else -(-nl // -(-nl // batch))
    touched = {(g, slots_of[s] // per) for g, st in enumerate(sets) for s in st}
    return 8 * n * sum(len(st) for st in sets) + 16 * n * len(touched)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--sets", type=int, default=1000)
    ap.add_argument("--pool", type=int, default=1000)
    ap.add_argument("--kg", type=int, nargs="+", default=[1, 10, 100])
    ap.add_argument("--host-sets", type=int, default=0, help="sets of leg (c); 0 (default): all of them, as the other legs")
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--epsilon", type=float, default=0.5)
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")

    import fora_amd
    from fora_amd import synth
    n, m, row_ptr, col = synth.preset(a.graph)
    deg = np.diff(row_ptr)
    eng = fora_amd.Engine(0)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    rng = np.random.Generator(np.random.PCG64(20261018))
    pool = rng.choice(np.flatnonzero(deg > 0), size=a.pool, replace=False).astype(np.int32)

    for kg in a.kg:
        sets = [rng.choice(pool, size=kg, replace=False).tolist() for _ in range(a.sets)]
        flat = (np.arange(a.sets + 1, dtype=np.int64) * kg, np.array(sets, dtype=np.int32).reshape(-1))
        host = sets[:max(1, min(a.host_sets, a.sets))] if a.host_sets > 0 else sets
        info = {}

        def leg_a():
            info["a"] = eng.query_seeds(flat, k=a.topk, want_fix=False)["stats"]
            return a.sets

        def leg_b():
            out = eng.query_seeds(flat, want_ppr=True, want_fix=False)
            info["dense_bytes"] = out["ppr"].nbytes
            return a.sets

        def leg_c():
            seeds = np.array(sorted({s for st in host for s in st}), dtype=np.int32)
            at = {int(s): i for i, s in enumerate(seeds)}
            rows, _ = eng.query(seeds, want_ppr=True)
            out = np.empty((len(host), n))
            w = np.full(kg, 1.0 / kg)
            for g, st in enumerate(host):
                np.dot(w, rows[[at[s] for s in st]], out=out[g])
            info["host_seeds"] = int(seeds.size)
            return len(host)

        def leg_d():
            eng.set_option("seeds_dedup", 0)
            try:
                info["d"] = eng.query_seeds(flat, k=a.topk, want_fix=False)["stats"]
            finally:
                eng.set_option("seeds_dedup", 1)
            return a.sets

        legs = [("seeds_topk", leg_a), ("seeds_dense_host", leg_b), ("host_sum", leg_c), ("seeds_topk_no_dedup", leg_d)]
        for _, f in legs:
            f()
        rate = {name: [] for name, _ in legs}
        combine = {"seeds_topk": [], "seeds_topk_no_dedup": []}
        batch_ms = {"seeds_topk": [], "seeds_topk_no_dedup": []}
        for _ in range(a.reps):
            for name, f in legs:
                eng.reset_timing()
                t0 = time.perf_counter()
                q = f()
                rate[name].append(q / (time.perf_counter() - t0))
                if name in combine:
                    combine[name].append(info["a" if name == "seeds_topk" else "d"]["combine_ms"])
                    batch_ms[name].append(eng.timing()["batch_ms"])
        st = info["a"]
        order = list(dict.fromkeys(s for s_ in sets for s in s_))
        nbytes = _combine_bytes(sets, {s: i for i, s in enumerate(order)}, max(1, eng.get_batch()), n)
        cms = statistics.median(combine["seeds_topk"])
        med = {k: statistics.median(v) for k, v in rate.items()}
        out = {
            "tool": "seeds_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "sets": a.sets, "k_g": kg, "pool": a.pool,
            "topk": a.topk, "host_sets": len(host), "host_seeds": info["host_seeds"], "like_for_like": len(host) == a.sets, "reps": a.reps,
            "seeds": int(st["seeds"]), "distinct": int(st["distinct"]), "queries": int(st["queries"]), "batches": int(st["batches"]),
            "queries_no_dedup": int(info["d"]["queries"]), "batches_no_dedup": int(info["d"]["batches"]),
            "sets_per_s": {k: _spread(v) for k, v in rate.items()},
            "ratio": {"a_over_c": round(med["seeds_topk"] / med["host_sum"], 2), "b_over_c": round(med["seeds_dense_host"] / med["host_sum"], 2),
                      "d_over_a": round(med["seeds_topk_no_dedup"] / med["seeds_topk"], 3)},
            "combine_ms": {k: _spread(v, 4) for k, v in combine.items()},
            "batch_ms": {k: round(statistics.median(v), 3) for k, v in batch_ms.items()},
            "combine_share_of_batch_ms": round(cms / statistics.median(batch_ms["seeds_topk"]), 5),
            "combine_bytes": int(nbytes), "combine_tb_per_s": round(nbytes / (cms * 1e-3) / 1e12, 3) if cms > 0 else None,
            "dense_host_bytes": int(info["dense_bytes"]),
        }
        print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
