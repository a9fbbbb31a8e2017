#!/usr/bin/env python3
"""Throughput of the reference's baselines on one GPU (optional tooling, not a yardstick): --algo montecarlo
(k_walk_mc: queries/s, walks/s and walk steps/s) and --algo fwdpush (the FORA push at fwdpush_setting's rmax:
queries/s) and --algo bippr (walks plus the n backward pushes of a call and their combine: queries/s and the split of
the time) on a synthetic R-MAT graph (default: the webstanford-sized preset, eps = 0.5).  One warm-up call, then the
timed calls; prints one JSON line.

    python tools/baseline_bench.py [--graph webstanford] [--mc-queries 170] [--fwd-queries 1000] [--bippr-queries 170] [--steps 2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--mc-queries", type=int, default=170, help="one batch of about this many slots at ws size")
    ap.add_argument("--fwd-queries", type=int, default=1000)
    ap.add_argument("--bippr-queries", type=int, default=170, help="sources per bippr call (one batch at ws size)")
    ap.add_argument("--steps", type=int, default=2)
    a = ap.parse_args()

    import fora_amd
    from fora_amd import synth
    n, m, rp, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    eng.set_graph(n, m, rp, col)
    eng.set_params(epsilon=a.epsilon, seed=0x464F5241)
    out = {"graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "batch": eng.get_batch()}

    srcs = synth.query_set(n, a.mc_queries, 7)
    eng.montecarlo(srcs[:2], epsilon=a.epsilon, want_fix=False)  # warm-up (workspace, code objects)
    eng.reset_timing()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        _, _, _, _, st = eng.montecarlo(srcs, epsilon=a.epsilon, want_fix=False)
    sec = time.perf_counter() - t0
    tm = eng.timing()
    q = a.steps * srcs.size
    out["mc"] = {"queries": int(srcs.size), "walks_per_query": int(st[0]["n_walks"]), "qps": q / sec,
                 "walks_per_s": tm["walks"] / sec, "steps_per_s": tm["walk_steps"] / sec,
                 "steps_per_walk": tm["walk_steps"] / max(1, tm["walks"]),
                 "kernel_steps_per_s": tm["walk_steps"] / (tm["walk_ms"] * 1e-3), "walk_ms": tm["walk_ms"],
                 "launches": tm["walk_launches"], "wall_s": sec}

    srcs = synth.query_set(n, a.fwd_queries, 8)
    eng.fwdpush(srcs[:2], epsilon=a.epsilon, want_fix=False)
    eng.reset_timing()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        eng.fwdpush(srcs, epsilon=a.epsilon, want_fix=False)
    sec = time.perf_counter() - t0
    tm = eng.timing()
    q = a.steps * srcs.size
    out["fwdpush"] = {"queries": int(srcs.size), "qps": q / sec, "pops": tm["pops"] // a.steps, "relax": tm["relax"] // a.steps,
                      "wall_s": sec}

    srcs = synth.query_set(n, a.bippr_queries, 9)
    eng.bippr(srcs[:2], epsilon=a.epsilon, want_fix=False)  # warm-up (reverse CSR, buffers)
    eng.reset_timing()
    bwds = []
    t0 = time.perf_counter()
    for _ in range(a.steps):
        _, _, _, _, st, bwd = eng.bippr(srcs, epsilon=a.epsilon, want_fix=False)
        bwds.append(bwd)
    sec = time.perf_counter() - t0
    tm = eng.timing()
    q = a.steps * srcs.size
    mean = lambda key: sum(b[key] for b in bwds) / len(bwds)  # noqa: E731
    out["bippr"] = {"queries": int(srcs.size), "qps": q / sec, "walks_per_query": int(st[0]["n_walks"]),
                    "rmax": float(st[0]["rmax_used"]), "bwd_ms_per_call": mean("bwd_ms"), "walk_ms_per_call": mean("walk_ms"),
                    "combine_ms_per_call": mean("combine_ms"), "entries": int(bwds[-1]["entries"]),
                    "global_targets": int(bwds[-1]["global_targets"]), "chunks": int(bwds[-1]["chunks"]),
                    "pops": int(bwds[-1]["pops"]), "relax": int(bwds[-1]["relax"]), "levels": int(bwds[-1]["levels"]),
                    "walks_per_s": tm["walks"] / sec, "wall_s": sec}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
