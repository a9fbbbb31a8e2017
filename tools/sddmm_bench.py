#!/usr/bin/env python3
"""What the operations with the caller's values on the held pattern cost: one held sparse result of
--queries sources -- the full thresholded rows (threshold 1 / n) and the rows cut to their --topk largest entries -- device
resident A [nq, d], B [n, d], values [entries], five legs,

  (a) sparse_sddmm                                     scores[e] = <A[row_e], B[id_e]>
  (b) sparse_propagate(values=)                        P(values) x B
  (c) sparse_propagate_t(values=), cached              P(values)^T x A, the transposition and pos already there
  (d) (A[row_of_entry] * B[ids]).sum(1)                the torch route to the scores on the same held rows: an entries x d gather
  (e) torch.sparse.sampled_addmm                       where this torch build has it for these tensors; "unavailable" otherwise

for d in --dims and the dense operands as float32 and bfloat16.  Every leg is warmed up once; then the legs run alternately
--reps times and the line carries each leg's median and spread (min, max) in ms per call.  Times are a host clock around
calls that end in a synchronise; sddmm_kernel_ms / gather_ms / combine_ms are the library's device events.

  python tools/sddmm_bench.py --graph webstanford
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
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--dims", default="64,128,256")
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")
    dims = [int(x) for x in a.dims.split(",")]

    import fora_amd
    from fora_amd import synth
    n, m, row_ptr, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    dev = torch.device("cuda", eng.device)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    srcs = synth.query_set(n, a.queries, 20261001)
    nq = len(srcs)
    rng = np.random.Generator(np.random.PCG64(20261019))

    for rows in ("thresholded", f"topk{a.topk}"):
        if rows == "thresholded":
            rp, ids, vals = eng.query_sparse(srcs, device=True)[:3]
        else:
            rp, ids, vals = eng.query_sparse_topk(srcs, a.topk, device=True)[:3]
        torch.cuda.synchronize()
        rp_host = rp.cpu().numpy()
        entries = int(rp_host[-1])
        lens = rp[1:] - rp[:-1]
        row_of = torch.repeat_interleave(torch.arange(nq, device=dev), lens, output_size=entries)
        ids64 = ids.to(torch.int64)
        values = torch.from_numpy(rng.standard_normal(entries, dtype=np.float32)).to(dev)
        info = {"sampled": None}

        def leg_sddmm(A, B):
            _, _, info["sddmm"] = eng.sparse_sddmm(rp_host, A, B)

        def leg_fwd(A, B):
            _, _, info["fwd"] = eng.sparse_propagate(rp_host, B, values=values)

        def leg_bwd(A, B):
            _, _, info["bwd"] = eng.sparse_propagate_t(rp_host, A, values=values)

        def leg_gather(A, B):
            (A[row_of] * B[ids64]).sum(1)
            torch.cuda.synchronize()

        def leg_sampled(A, B):
            if info["sampled"] is None:
                try:
                    pattern = torch.sparse_csr_tensor(rp, ids64, torch.zeros(entries, dtype=A.dtype, device=dev), size=(nq, n))
                    torch.sparse.sampled_addmm(pattern, A, B.t(), beta=0.0)
                    torch.cuda.synchronize()
                except Exception as e:
                    info["sampled"] = f"unavailable: {type(e).__name__}: {str(e)[:160]}"

        for d in dims:
            A32 = torch.from_numpy(rng.standard_normal((nq, d), dtype=np.float32)).to(dev)
            B32 = torch.from_numpy(rng.standard_normal((n, d), dtype=np.float32)).to(dev)
            for dtype, A, B in (("f32", A32, B32), ("bf16", A32.to(torch.bfloat16), B32.to(torch.bfloat16))):
                info["sampled"] = None                       # (a build may have the kernel for one type only: tried again per case)
                legs = [("sddmm", leg_sddmm), ("propagate_vals", leg_fwd), ("propagate_t_vals", leg_bwd), ("torch_gather_dot", leg_gather),
                        ("torch_sampled_addmm", leg_sampled)]
                for _, f in legs:
                    f(A, B)
                ms = {name: [] for name, _ in legs}
                ev = {k: [] for k in ("sddmm_kernel", "fwd_gather", "fwd_combine", "bwd_gather", "bwd_combine")}
                for _ in range(a.reps):
                    for name, f in legs:
                        t0 = time.perf_counter()
                        f(A, B)
                        ms[name].append((time.perf_counter() - t0) * 1e3)
                    ev["sddmm_kernel"].append(info["sddmm"]["sddmm_ms"])
                    ev["fwd_gather"].append(info["fwd"]["gather_ms"]); ev["fwd_combine"].append(info["fwd"]["combine_ms"])
                    ev["bwd_gather"].append(info["bwd"]["gather_ms"]); ev["bwd_combine"].append(info["bwd"]["combine_ms"])
                sampled = info["sampled"] or "ok"
                if sampled != "ok":
                    ms.pop("torch_sampled_addmm")
                out = {"tool": "sddmm_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "queries": a.queries, "reps": a.reps,
                       "rows": rows, "d": d, "operands": dtype, "entries": entries, "segments": int(info["sddmm"]["segments"]),
                       "max_row": int(info["sddmm"]["max_row"]), "sddmm_bytes": int(info["sddmm"]["bytes"]),
                       "ms": {k: _summary(v) for k, v in ms.items()},
                       "sddmm_kernel_ms": _summary(ev["sddmm_kernel"], 4),
                       "fwd_gather_ms": _summary(ev["fwd_gather"], 4), "fwd_combine_ms": _summary(ev["fwd_combine"], 4),
                       "bwd_gather_ms": _summary(ev["bwd_gather"], 4), "bwd_combine_ms": _summary(ev["bwd_combine"], 4),
                       "torch_sampled_addmm": sampled}
                print(json.dumps(out), flush=True)
            del A32, B32
    eng.close()


if __name__ == "__main__":
    main()
