#!/usr/bin/env python3
"""Targeted BiPPR against the single-source form on one GPU (optional tooling, not a yardstick): Engine.bippr (n backward
pushes per call) and Engine.bippr_targets with nt random targets, an rmax_scale sweep at nt = 100, and the heavy-target
case (the node of largest in-degree as the only target, 64 sources) through the library's choice of lane mapping and span,
through lane = entry, and through lane = slot with one span over the whole target, the one-wave-per-target shape of
k_bippr_combine.  Every leg is warmed up once, then the legs run alternately `--reps` times in one process; prints one JSON
line with median [min, max] per leg.

    python tools/bippr_targets_bench.py [--graph webstanford] [--queries 1000] [--reps 3]
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


def _mmm(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-full", action="store_true", help="skip the single-source leg")
    a = ap.parse_args()

    import fora_amd
    from fora_amd import synth
    n, m, rp, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    eng.set_graph(n, m, rp, col)
    eng.set_params(epsilon=a.epsilon, seed=0x464F5241)
    srcs = synth.query_set(n, a.queries, 9)
    rng = np.random.Generator(np.random.PCG64(11))
    hub = int(np.bincount(col[:int(rp[-1])], minlength=n).argmax())

    legs = []  # (name, sources, call, options)
    if not a.no_full:
        legs.append(("full", srcs, lambda: eng.bippr(srcs, epsilon=a.epsilon, want_fix=False)[4:], {}))
    for nt in (1, 100, 10000):
        tg = rng.integers(0, n, size=nt).astype(np.int32)
        legs.append((f"targets_{nt}", srcs, lambda tg=tg: eng.bippr_targets(srcs, tg, epsilon=a.epsilon)[2:], {}))
        if nt == 100:
            for sc in (0.1, 0.01):
                legs.append((f"targets_100_scale_{sc}", srcs,
                             lambda tg=tg, sc=sc: eng.bippr_targets(srcs, tg, epsilon=a.epsilon, rmax_scale=sc)[2:], {}))
    s64 = srcs[:64]
    one = np.array([hub], dtype=np.int32)
    heavy = lambda: eng.bippr_targets(s64, one, epsilon=a.epsilon)[2:]  # noqa: E731
    legs.append(("heavy_auto", s64, heavy, {}))
    legs.append(("heavy_by_entry", s64, heavy, {"tgt_lanes": 1}))
    legs.append(("heavy_one_wave", s64, heavy, {"tgt_lanes": 0, "tgt_span": 1 << 30}))

    def run(call, opts):
        for k, v in opts.items():
            eng.set_option(k, v)
        t0 = time.perf_counter()
        st, bwd = call()
        sec = time.perf_counter() - t0
        for k in opts:
            eng.set_option(k, -1 if k == "tgt_lanes" else 0)
        return sec, st, bwd

    for _, _, call, opts in legs:  # warm-up (reverse CSR, buffers, code objects)
        run(call, opts)
    acc = {name: {"qps": [], "wall_ms": [], "bwd_ms": [], "walk_ms": [], "combine_ms": []} for name, _, _, _ in legs}
    last = {}
    for _ in range(a.reps):
        for name, ss, call, opts in legs:
            sec, st, bwd = run(call, opts)
            r = acc[name]
            r["qps"].append(len(ss) / sec)
            r["wall_ms"].append(sec * 1e3)
            for k in ("bwd_ms", "walk_ms", "combine_ms"):
                r[k].append(bwd[k])
            last[name] = (st, bwd)
    out = {"tool": "bippr_targets_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "queries": int(srcs.size),
           "reps": a.reps, "hub": hub, "legs": {}}
    for name, ss, _, _ in legs:
        st, bwd = last[name]
        leg = {k: _mmm(v) for k, v in acc[name].items()}
        leg.update(sources=len(ss), walks_per_query=int(st[0]["n_walks"]), rmax=float(st[0]["rmax_used"]),
                   targets=int(bwd["targets"]), entries=int(bwd["entries"]), pops=int(bwd["pops"]), relax=int(bwd["relax"]),
                   global_targets=int(bwd["global_targets"]), levels=int(bwd["levels"]), chunks=int(bwd["chunks"]))
        out["legs"][name] = leg
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
