#!/usr/bin/env python3
"""What the top-k rows cost and what they buy: the same sources through these legs, one process,

  hbm_only            query(want_ppr=False)                          the vectors stay in HBM (what bench.py times)
  sparse_device       query_sparse(device=True) at 1/n               the full thresholded rows
  topk_K              query_sparse_topk(k=K, device=True), K of --ks the rows cut to their K largest entries on the GPU
  sparse_torch_topk   query_sparse(device=True), then torch.topk     a user's alternative: the full rows padded to the longest
                      over the padded rows (k = the first of --ks)   one on the device and cut there

Every leg is warmed up once; then the legs run alternately --reps times and the line carries each leg's median and spread
(min, max) in queries/s: a difference smaller than the spread is not a difference.  Times are a host clock around calls that
end in a stream synchronise; select_ms, compact_ms and gather_ms are the library's device events.  gather_ms: one
sparse_propagate with d = 128 float32 features on the device over the held rows of the leg.

  python tools/sparse_topk_bench.py --graph webstanford
  python tools/sparse_topk_bench.py --graph livejournal --with-idx
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before the library is loaded: one HIP runtime in the process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--with-idx", action="store_true")
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--ks", default="32,256,2048")
    ap.add_argument("--d", type=int, default=128)
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")
    ks = [int(x) for x in a.ks.split(",")]

    import fora_amd
    from fora_amd import synth
    n, m, row_ptr, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    dev = torch.device("cuda", eng.device)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    if a.with_idx:
        eng.build_index()
    srcs = synth.query_set(n, a.queries, 20261001)
    H = torch.randn((n, a.d), dtype=torch.float32, device=dev)
    info = {}

    def gather(rp, key):
        _, _, ps = eng.sparse_propagate(rp, H)
        info.setdefault("gather_ms", {}).setdefault(key, []).append(ps["gather_ms"])

    def leg_hbm():
        eng.query(srcs, with_idx=a.with_idx, want_ppr=False)

    def leg_sparse():
        rp, ids, vals, st, sp = eng.query_sparse(srcs, with_idx=a.with_idx, device=True)
        torch.cuda.synchronize()
        info["sp"] = sp
        return rp

    def leg_topk(k):
        def run():
            rp, ids, vals, st, sp, tk = eng.query_sparse_topk(srcs, k, with_idx=a.with_idx, device=True)
            torch.cuda.synchronize()
            r = info.setdefault("topk", {}).setdefault(str(k), {"select_ms": [], "compact_ms": []})
            r["select_ms"].append(tk["select_ms"])
            r["compact_ms"].append(sp["compact_ms"])
            r.update(entries=int(sp["entries"]), max_row=int(sp["max_row"]), support=int(tk["support"]), max_support=int(tk["max_support"]),
                     cut_rows=tk["cut_rows"], lds_rows=tk["lds_rows"], global_rows=tk["global_rows"], chunks=tk["chunks"])
            return rp
        return run

    def leg_torch():
        k = ks[0]
        rp, ids, vals, st, sp = eng.query_sparse(srcs, with_idx=a.with_idx, device=True)
        lens = rp[1:] - rp[:-1]
        width = int(lens.max())
        pos = torch.arange(width, device=dev)[None, :]
        live = pos < lens[:, None]
        at = (rp[:-1, None] + pos).clamp_(max=max(int(rp[-1]) - 1, 0))
        padded = torch.where(live, vals[at], torch.full((), -1.0, dtype=vals.dtype, device=dev))
        top = torch.topk(padded, min(k, width), dim=1)
        info["torch_ids"] = torch.gather(ids[at], 1, top.indices)
        torch.cuda.synchronize()

    legs = [("hbm_only", leg_hbm), ("sparse_device", leg_sparse)] + [(f"topk_{k}", leg_topk(k)) for k in ks] + [("sparse_torch_topk", leg_torch)]
    for _, f in legs:
        f()
    for v in info.get("topk", {}).values():   # the warm-up's events do not count
        v["select_ms"].clear(); v["compact_ms"].clear()
    qps = {name: [] for name, _ in legs}
    for _ in range(a.reps):
        for name, f in legs:
            t0 = time.perf_counter()
            rp = f()
            qps[name].append(a.queries / (time.perf_counter() - t0))
            if rp is not None:
                gather(rp, name)
    topk = {k: {**v, "select_ms": spread(v["select_ms"], 4), "compact_ms": spread(v["compact_ms"], 4)} for k, v in info["topk"].items()}
    out = {
        "tool": "sparse_topk_bench", "graph": a.graph, "n": n, "m": m, "with_idx": bool(a.with_idx), "epsilon": a.epsilon,
        "queries": a.queries, "reps": a.reps, "threshold": "1/n", "d": a.d,
        "qps": {k: spread(v) for k, v in qps.items()},
        "full_rows": {"entries": int(info["sp"]["entries"]), "max_row": int(info["sp"]["max_row"]), "compact_ms": info["sp"]["compact_ms"]},
        "topk": topk,
        "gather_ms": {k: spread(v, 4) for k, v in info["gather_ms"].items()},
    }
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
