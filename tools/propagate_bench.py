#!/usr/bin/env python3
"""What feature propagation costs beside the query that makes its rows: the same sources through four legs,
one process, device-resident features H [n, d],

  (a) query_sparse(device=True)                          the rows alone, fetched into torch tensors on the GPU
  (b) (a) + sparse_propagate                             the library's ordered product, out32 on the GPU
  (c) (a) + torch.sparse.mm(to_torch_csr(...), H f64)    what a caller could do before: a generic SpMM, bits undefined
  (d) query_sparse to host arrays + numpy                per row vals @ H[ids], on --host-rows rows only: the figure
                                                         "host_numpy_scaled_to_queries" is that time scaled to
                                                         --queries rows, an extrapolation and not a measurement

for d in --dims and H as float32 and bfloat16.  Every leg is warmed up once; then the legs run alternately --reps times and
the line carries each leg's median and spread (min, max) in ms per call: a difference smaller than the spread is not a
difference.  Times are a host clock around calls that end in a synchronise; gather_ms / combine_ms are the library's device
events, bytes_per_s = feat_bytes / gather time.  If this torch build cannot run leg (c) the line says so.

  python tools/propagate_bench.py --graph webstanford
  python tools/propagate_bench.py --graph livejournal --with-idx
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
    ap.add_argument("--host-rows", type=int, default=32, help="rows of the host leg (d)")
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
    info = {"spmm_error": None}

    def rows():
        out = eng.query_sparse(srcs, with_idx=a.with_idx, device=True)
        torch.cuda.synchronize()
        info["sp"] = out[4]
        return out[:3]

    def leg_rows(H, H64):
        rows()

    def leg_prop(H, H64):
        rp, ids, vals = rows()
        _, _, info["ps"] = eng.sparse_propagate(rp, H)

    def leg_spmm(H, H64):
        rp, ids, vals = rows()
        if info["spmm_error"] is None:
            try:
                torch.sparse.mm(capi.to_torch_csr(rp, ids, vals, n), H64)
                torch.cuda.synchronize()
            except Exception as e:  # this torch build has no CSR SpMM for the device: said in the line, not fatal
                info["spmm_error"] = f"{type(e).__name__}: {str(e)[:200]}"

    def leg_host(H, H64):
        rp, ids, vals, st, sp = eng.query_sparse(srcs[:a.host_rows], with_idx=a.with_idx)
        Hh = info["H_host"]
        out = np.zeros((a.host_rows, Hh.shape[1]))
        for i in range(len(rp) - 1):
            out[i] = vals[rp[i]:rp[i + 1]] @ Hh[ids[rp[i]:rp[i + 1]]].astype(np.float64)

    for d in dims:
        Hh = rng.standard_normal((n, d), dtype=np.float32)
        info["H_host"] = Hh
        H32 = torch.from_numpy(Hh).to(dev)
        H64 = H32.to(torch.float64)
        for dtype, H in (("f32", H32), ("bf16", H32.to(torch.bfloat16))):
            legs = [("rows", leg_rows), ("rows_propagate", leg_prop), ("rows_torch_spmm", leg_spmm)] + ([("host_numpy", leg_host)] if dtype == "f32" else [])
            for _, f in legs:
                f(H, H64)
            ms = {name: [] for name, _ in legs}
            gather, combine, alone = [], [], []
            for _ in range(a.reps):
                for name, f in legs:
                    t0 = time.perf_counter()
                    f(H, H64)
                    ms[name].append((time.perf_counter() - t0) * 1e3)
                    if name == "rows_propagate":
                        gather.append(info["ps"]["gather_ms"])
                        combine.append(info["ps"]["combine_ms"])
                        rp = eng.query_sparse(srcs, with_idx=a.with_idx, device=True)[0]   # the call alone, on a held result
                        t1 = time.perf_counter()
                        eng.sparse_propagate(rp, H)
                        alone.append((time.perf_counter() - t1) * 1e3)
            ps = info["ps"]
            g = statistics.median(gather)
            out = {"tool": "propagate_bench", "graph": a.graph, "n": n, "m": m, "with_idx": bool(a.with_idx), "epsilon": a.epsilon,
                   "queries": a.queries, "reps": a.reps, "threshold": "1/n", "d": d, "feat": dtype,
                   "entries": int(ps["entries"]), "segments": int(ps["segments"]), "max_row": int(ps["max_row"]), "chunks": int(ps["chunks"]),
                   "feat_bytes": int(ps["feat_bytes"]), "ms": {k: _summary(v) for k, v in ms.items()},
                   "propagate_alone_ms": _summary(alone), "gather_ms": _summary(gather, 4), "combine_ms": _summary(combine, 4),
                   "gather_bytes_per_s": round(ps["feat_bytes"] / (g * 1e-3), 0) if g > 0 else None,
                   "host_rows": a.host_rows if dtype == "f32" else None, "torch_spmm": info["spmm_error"] or "ok"}
            if "host_numpy" in ms:
                out["ms"]["host_numpy_scaled_to_queries"] = round(statistics.median(ms["host_numpy"]) * a.queries / a.host_rows, 1)
            print(json.dumps(out), flush=True)
        del H32, H64
    eng.close()


if __name__ == "__main__":
    main()
