#!/usr/bin/env python3
"""What the backward pass of feature propagation costs beside the forward pass: one held sparse result
(query_sparse of --queries sources at threshold 1 / n, made once), device-resident H [n, d] and G [nq, d], four legs,

  (a) sparse_propagate                                     the forward product on the held result (the figures of 5.12)
  (b) sparse_propagate_t, first call                       the option "propt_lds_cap" is set to another value and back before
                                                           it, which drops the cached transposition: transpose_ms is the
                                                           build (count, the host's prefix sum, place, sort, fill)
  (c) sparse_propagate_t, cached                           what every later backward pass costs
  (d) torch.sparse.mm(to_torch_csr(...).t() as CSR, G f64) what a caller could do before; the transposition by torch is timed
                                                           once on its own (torch_transpose_ms) and kept

for d in --dims and G as float32 and bfloat16.  Every leg is warmed up once; then the legs run alternately --reps times and
the line carries each leg's median and spread (min, max) in ms per call.  Times are a host clock around calls that end in a
synchronise; transpose_ms / gather_ms / combine_ms are the library's device events.

  python tools/propagate_t_bench.py --graph webstanford
  python tools/propagate_t_bench.py --graph livejournal --with-idx
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


def _summary(v, digits=3):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--with-idx", action="store_true")
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--dims", default="64,128,256")
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")
    dims = [int(x) for x in a.dims.split(",")]

    import fora_amd
    from fora_amd import capi, synth
    n, m, row_ptr, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    dev = torch.device("cuda", eng.device)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    if a.with_idx:
        eng.build_index()
    srcs = synth.query_set(n, a.queries, 20261001)
    rng = np.random.Generator(np.random.PCG64(20261019))
    rp, ids, vals, st, sp = eng.query_sparse(srcs, with_idx=a.with_idx, device=True)
    torch.cuda.synchronize()
    nq = len(srcs)
    cap = eng.get_option("propt_lds_cap")
    info = {"spmm_error": None, "At": None, "torch_transpose_ms": None}
    try:
        t0 = time.perf_counter()
        info["At"] = capi.to_torch_csr(rp, ids, vals, n).t().to_sparse_csr()
        torch.cuda.synchronize()
        info["torch_transpose_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    except Exception as e:  # this torch build cannot transpose a CSR on the device: said in the line, not fatal
        info["spmm_error"] = f"{type(e).__name__}: {str(e)[:200]}"

    def leg_forward(H, G, G64):
        _, _, info["fwd"] = eng.sparse_propagate(rp, H)

    def leg_first(H, G, G64):
        eng.set_option("propt_lds_cap", cap - 1)
        eng.set_option("propt_lds_cap", cap)
        _, _, info["first"] = eng.sparse_propagate_t(rp, G)
        assert info["first"]["built"] == 1

    def leg_cached(H, G, G64):
        _, _, info["bwd"] = eng.sparse_propagate_t(rp, G)
        assert info["bwd"]["built"] == 0

    def leg_spmm(H, G, G64):
        if info["spmm_error"] is None:
            try:
                torch.sparse.mm(info["At"], G64)
                torch.cuda.synchronize()
            except Exception as e:
                info["spmm_error"] = f"{type(e).__name__}: {str(e)[:200]}"

    for d in dims:
        H32 = torch.from_numpy(rng.standard_normal((n, d), dtype=np.float32)).to(dev)
        G32 = torch.from_numpy(rng.standard_normal((nq, d), dtype=np.float32)).to(dev)
        G64 = G32.to(torch.float64)
        for dtype, H, G in (("f32", H32, G32), ("bf16", H32.to(torch.bfloat16), G32.to(torch.bfloat16))):
            legs = [("forward", leg_forward), ("backward_first", leg_first), ("backward_cached", leg_cached), ("torch_spmm_t", leg_spmm)]
            for _, f in legs:
                f(H, G, G64)
            ms = {name: [] for name, _ in legs}
            ev = {k: [] for k in ("fwd_gather", "fwd_combine", "transpose", "gather", "combine")}
            for _ in range(a.reps):
                for name, f in legs:
                    t0 = time.perf_counter()
                    f(H, G, G64)
                    ms[name].append((time.perf_counter() - t0) * 1e3)
                ev["fwd_gather"].append(info["fwd"]["gather_ms"]); ev["fwd_combine"].append(info["fwd"]["combine_ms"])
                ev["transpose"].append(info["first"]["transpose_ms"])
                ev["gather"].append(info["bwd"]["gather_ms"]); ev["combine"].append(info["bwd"]["combine_ms"])
            first, bwd = info["first"], info["bwd"]
            out = {"tool": "propagate_t_bench", "graph": a.graph, "n": n, "m": m, "with_idx": bool(a.with_idx), "epsilon": a.epsilon,
                   "queries": a.queries, "reps": a.reps, "threshold": "1/n", "d": d, "grad": dtype,
                   "entries": int(bwd["entries"]), "columns": int(bwd["columns"]), "segments": int(bwd["segments"]), "max_col": int(bwd["max_col"]),
                   "fwd_segments": int(info["fwd"]["segments"]), "chunks": int(bwd["chunks"]),
                   "short_cols": int(first["short_cols"]), "lds_cols": int(first["lds_cols"]), "global_cols": int(first["global_cols"]),
                   "ms": {k: _summary(v) for k, v in ms.items()},
                   "fwd_gather_ms": _summary(ev["fwd_gather"], 4), "fwd_combine_ms": _summary(ev["fwd_combine"], 4),
                   "transpose_ms": _summary(ev["transpose"], 4), "gather_ms": _summary(ev["gather"], 4), "combine_ms": _summary(ev["combine"], 4),
                   "torch_transpose_ms": info["torch_transpose_ms"], "torch_spmm": info["spmm_error"] or "ok"}
            print(json.dumps(out), flush=True)
        del H32, G32, G64
    eng.close()


if __name__ == "__main__":
    main()
