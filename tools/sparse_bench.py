#!/usr/bin/env python3
"""What the sparse result costs and what it buys ("Sparse results"): the same sources through four legs, one process,

  (a) query(want_ppr=False)                  the vectors stay in HBM (what bench.py times)
  (b) query_sparse at 1/n, fetched to host   thresholded CSR, compacted on the GPU
  (c) query_sparse(device=True)              the same, fetched into torch tensors on the GPU
  (d) query(want_ppr=True)                   the dense nq * n array, on as many sources as fit --dense-bytes of host memory

Every leg is warmed up once; then the legs run alternately --reps times and the line carries each leg's median and
spread (min, max) in queries/s: a difference smaller than the spread is not a difference.  Times are a host clock around
calls that end in a stream synchronise; compact_ms and batch_ms are the library's device events.

  python tools/sparse_bench.py --graph webstanford
  python tools/sparse_bench.py --graph livejournal --with-idx          (BASELINE config 3)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before the library is loaded: one HIP runtime in the process (Engine.query_sparse, device=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--with-idx", action="store_true")
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--dense-bytes", type=float, default=4e9, help="host memory the dense leg may fill")
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")

    import fora_amd
    from fora_amd import synth
    n, m, row_ptr, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    if a.with_idx:
        eng.build_index()
    srcs = synth.query_set(n, a.queries, 20261001)
    nd = int(max(1, min(a.queries, a.dense_bytes // (8 * n))))
    info = {}

    def leg_a():
        eng.query(srcs, with_idx=a.with_idx, want_ppr=False)
        return a.queries

    def leg_b():
        rp, ids, vals, st, sp = eng.query_sparse(srcs, with_idx=a.with_idx)
        info["sp"] = sp
        info["rows"] = np.diff(rp)
        info["host_bytes"] = rp.nbytes + ids.nbytes + vals.nbytes
        return a.queries

    def leg_c():
        rp, ids, vals, st, sp = eng.query_sparse(srcs, with_idx=a.with_idx, device=True)
        torch.cuda.synchronize()
        info["device_bytes"] = (rp.numel() + vals.numel()) * 8 + ids.numel() * 4
        info["compact_ms_c"] = sp["compact_ms"]
        return a.queries

    def leg_d():
        out, _ = eng.query(srcs[:nd], with_idx=a.with_idx, want_ppr=True)
        info["dense_bytes"] = out.nbytes
        return nd

    legs = [("hbm_only", leg_a), ("sparse_host", leg_b), ("sparse_device", leg_c), ("dense_host", leg_d)]
    for _, f in legs:
        f()
    qps = {name: [] for name, _ in legs}
    compact, batch_ms = [], []
    for _ in range(a.reps):
        for name, f in legs:
            eng.reset_timing()
            t0 = time.perf_counter()
            q = f()
            qps[name].append(q / (time.perf_counter() - t0))
            if name == "sparse_host":
                compact.append(info["sp"]["compact_ms"])
                batch_ms.append(eng.timing()["batch_ms"])
    rows = info["rows"]
    out = {
        "tool": "sparse_bench", "graph": a.graph, "n": n, "m": m, "with_idx": bool(a.with_idx), "epsilon": a.epsilon,
        "queries": a.queries, "dense_queries": nd, "reps": a.reps, "threshold": "1/n", "thr_fix": info["sp"]["thr_fix"],
        "batches": info["sp"]["batches"],
        "qps": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in qps.items()},
        "compact_ms": {"median": round(statistics.median(compact), 4), "min": round(min(compact), 4), "max": round(max(compact), 4)},
        "batch_ms": round(statistics.median(batch_ms), 3),
        "entries": int(info["sp"]["entries"]), "entries_per_row": {"mean": round(float(rows.mean()), 1), "max": int(rows.max())},
        "bytes_fetched": {"sparse_host": int(info["host_bytes"]), "sparse_device": int(info["device_bytes"]),
                          "dense_host": int(info["dense_bytes"]), "dense_host_at_all_queries": int(8 * n * a.queries)},
    }
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
