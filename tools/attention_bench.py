#!/usr/bin/env python3
"""What attention over the held rows costs in one call and in three: one held sparse result of --queries
sources -- the full thresholded rows (threshold 1 / n: nearly all longer than 256 entries, the chained path inside the call) and
the rows cut to their --topk largest entries (the fused kernel) -- device resident float32 Q [nq, heads * d], K [n, heads * d],
V [n, heads * d] for every head count of --heads, and the legs

  (a) sparse_attention                                      the one call, float32 out and float32 y
  (b) sparse_sddmm, sparse_softmax, sparse_propagate        the three calls chained through float64, once per head on column slices
  (c) ppr_attention(softmax="engine"), forward + backward   one head per call, once per head on column slices
  (d) ppr_attention_fused, forward + backward               all heads in one forward call

Every leg is warmed up once; then the legs run alternately --reps times and the line carries each leg's median and spread
(min, max) in ms per call.  Times are a host clock around calls that end in a synchronise; attn_kernel_ms is the library's
device events around the launches of (a), chained_kernel_ms the sum of the three calls' device events of (b).

  python tools/attention_bench.py --graph webstanford
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--heads", type=int, nargs="+", default=[1, 8])
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")

    import fora_amd
    from fora_amd import synth
    from fora_amd.torch_ops import ppr_attention, ppr_attention_fused
    n, m, row_ptr, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    dev = torch.device("cuda", eng.device)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    srcs = synth.query_set(n, a.queries, 20261001)
    nq = len(srcs)
    rng = np.random.Generator(np.random.PCG64(20261020))
    d = a.d
    scale = float(d) ** -0.5

    for rows in ("thresholded", f"topk{a.topk}"):
        if rows == "thresholded":
            rp = eng.query_sparse(srcs, device=True)[0]
        else:
            rp = eng.query_sparse_topk(srcs, a.topk, device=True)[0]
        torch.cuda.synchronize()
        rp_host = rp.cpu().numpy()
        entries = int(rp_host[-1])
        for heads in a.heads:
            w = heads * d
            Q = torch.from_numpy(rng.standard_normal((nq, w), dtype=np.float32)).to(dev).requires_grad_(True)
            K = torch.from_numpy(rng.standard_normal((n, w), dtype=np.float32)).to(dev).requires_grad_(True)
            V = torch.from_numpy(rng.standard_normal((n, w), dtype=np.float32)).to(dev).requires_grad_(True)
            G = torch.from_numpy(rng.standard_normal((nq, w), dtype=np.float32)).to(dev)
            Qd, Kd, Vd = Q.detach(), K.detach(), V.detach()
            out64 = torch.empty((nq, w), dtype=torch.float64, device=dev)
            info = {}

            def leg_fused():
                _, _, _, _, info["fused"] = eng.sparse_attention(rp_host, Qd, Kd, Vd, heads=heads, scale=scale, want_y32=True)

            def leg_chained():
                ms = 0.0
                for j in range(heads):
                    cs = slice(j * d, (j + 1) * d)
                    _, s64, st1 = eng.sparse_sddmm(rp_host, Qd[:, cs], Kd[:, cs], want32=False, want64=True)
                    _, y64, st2 = eng.sparse_softmax(rp_host, s64, scale=scale, want32=False, want64=True)
                    _, _, st3 = eng.sparse_propagate(rp_host, Vd[:, cs], want32=False, out64=out64[:, cs], values=y64)
                    ms += st1["sddmm_ms"] + st2["softmax_ms"] + st3["gather_ms"] + st3["combine_ms"]
                info["chained_ms"] = ms

            def leg_engine_fwd_bwd():
                for x in (Q, K, V):
                    x.grad = None
                outs = [ppr_attention(eng, rp_host, Q[:, j * d:(j + 1) * d], K[:, j * d:(j + 1) * d], V[:, j * d:(j + 1) * d], scale=scale, softmax="engine")
                        for j in range(heads)]
                torch.cat(outs, dim=1).backward(G)
                torch.cuda.synchronize()

            def leg_fused_fwd_bwd():
                for x in (Q, K, V):
                    x.grad = None
                ppr_attention_fused(eng, rp_host, Q, K, V, scale=scale, heads=heads).backward(G)
                torch.cuda.synchronize()

            legs = [("attention_one_call", leg_fused), ("attention_three_calls", leg_chained),
                    ("fwd_bwd_engine", leg_engine_fwd_bwd), ("fwd_bwd_fused", leg_fused_fwd_bwd)]
            for _, f in legs:
                f()
            ms = {name: [] for name, _ in legs}
            ev = {"attn_kernel": [], "chained_kernel": []}
            for _ in range(a.reps):
                for name, f in legs:
                    t0 = time.perf_counter()
                    f()
                    ms[name].append((time.perf_counter() - t0) * 1e3)
                ev["attn_kernel"].append(info["fused"]["attn_ms"])
                ev["chained_kernel"].append(info["chained_ms"])
            st = info["fused"]
            out = {"tool": "attention_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "queries": a.queries, "reps": a.reps,
                   "rows": rows, "d": d, "dv": d, "heads": heads, "entries": entries, "segments": int(st["segments"]), "max_row": int(st["max_row"]),
                   "short_rows": int(st["short_rows"]), "long_rows": int(st["long_rows"]), "nan_rows": int(st["nan_rows"]),
                   "ms": {k: _summary(v) for k, v in ms.items()},
                   "attn_kernel_ms": _summary(ev["attn_kernel"], 4), "chained_kernel_ms": _summary(ev["chained_kernel"], 4)}
            print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
