#!/usr/bin/env python3
"""What the backward pass of attention over the held rows costs in one call and in five per head: one held
sparse result of --queries sources -- the full thresholded rows (threshold 1 / n: nearly all longer than 256 entries, the chained
kernels inside the call) and the rows cut to their --topk largest entries (the fused kernels) -- device resident float32 Q
[nq, heads * d], K [n, heads * d], V [n, heads * d], G [nq, heads * d] and the float32 y of the forward call, for every head count
of --heads, and the legs

  (a) sparse_attention_bwd                                          the one call, float32 dq, dk and dv, the column plan cached
  (b) sparse_propagate_t, sparse_sddmm, sparse_softmax_bwd,         the five existing calls per head on column slices, as
      sparse_propagate, sparse_propagate_t                          ppr_attention_fused(backward="calls") makes them
  (c) ppr_attention_fused(backward="calls"), forward + backward
  (d) ppr_attention_fused(backward="fused"), forward + backward

Every leg is warmed up once; then the legs run alternately --reps times and the line carries each leg's median and spread
(min, max) in ms per call.  Times are a host clock around calls that end in a synchronise; bwd_kernel_ms is the library's device
events around the launches of (a).  first_call_ms is (a) on rows that have just become held -- the transposition, its places and
the column plan are made inside the call -- and replan_ms is (a) after the option "attn_short" changed: the column plan alone.
Both need the rows held again (a query), so they are measured --first times before the alternating legs.

  python tools/attention_bwd_bench.py --graph webstanford
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
    ap.add_argument("--with-idx", action="store_true", help="build the walk index first (the large presets)")
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=64)
    ap.add_argument("--rows", nargs="+", default=["thresholded", "topk"], choices=["thresholded", "topk"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--first", type=int, default=3)
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--heads", type=int, nargs="+", default=[1, 8])
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")

    import fora_amd
    from fora_amd import synth
    from fora_amd.torch_ops import ppr_attention_fused
    n, m, row_ptr, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    dev = torch.device("cuda", eng.device)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    if a.with_idx:
        eng.build_index()
    srcs = synth.query_set(n, a.queries, 20261001)
    nq = len(srcs)
    rng = np.random.Generator(np.random.PCG64(20261020))
    d = a.d
    scale = float(d) ** -0.5

    def hold(rows):
        if rows == "thresholded":
            rp = eng.query_sparse(srcs, with_idx=a.with_idx, device=True)[0]
        else:
            rp = eng.query_sparse_topk(srcs, a.topk, with_idx=a.with_idx, device=True)[0]
        torch.cuda.synchronize()
        return rp.cpu().numpy()

    for rows in a.rows:
        rp_host = hold(rows)
        entries = int(rp_host[-1])
        for heads in a.heads:
            w = heads * d
            Q = torch.from_numpy(rng.standard_normal((nq, w), dtype=np.float32)).to(dev).requires_grad_(True)
            K = torch.from_numpy(rng.standard_normal((n, w), dtype=np.float32)).to(dev).requires_grad_(True)
            V = torch.from_numpy(rng.standard_normal((n, w), dtype=np.float32)).to(dev).requires_grad_(True)
            G = torch.from_numpy(rng.standard_normal((nq, w), dtype=np.float32)).to(dev)
            Qd, Kd, Vd = Q.detach(), K.detach(), V.detach()
            dQ, dK, dV = torch.empty_like(Qd), torch.empty_like(Kd), torch.empty_like(Vd)
            info = {}

            def leg_one_call():
                info["bwd"] = eng.sparse_attention_bwd(rp_host, Qd, Kd, Vd, G, y32, heads=heads, scale=scale, dq32=dQ, dk32=dK, dv32=dV)[6]

            def leg_five_calls():
                for j in range(heads):
                    cs = slice(j * d, (j + 1) * d)
                    Gj, yj = G[:, cs], y32[j]
                    eng.sparse_propagate_t(rp_host, Gj, want64=False, values=yj, out32=dV[:, cs])
                    dy, _, _ = eng.sparse_sddmm(rp_host, Gj, Vd[:, cs], want32=True, want64=False)
                    ds, _, _ = eng.sparse_softmax_bwd(rp_host, yj, dy, scale=scale, want32=True, want64=False)
                    eng.sparse_propagate(rp_host, Kd[:, cs], want64=False, values=ds, out32=dQ[:, cs])
                    eng.sparse_propagate_t(rp_host, Qd[:, cs], want64=False, values=ds, out32=dK[:, cs])

            def fwd_bwd(backward):
                for x in (Q, K, V):
                    x.grad = None
                ppr_attention_fused(eng, rp_host, Q, K, V, scale=scale, heads=heads, backward=backward).backward(G)
                torch.cuda.synchronize()

            # ---- the first call on rows that have just become held, and the call that plans the columns again
            first, replan, first_st = [], [], None
            for _ in range(a.first):
                rp_host = hold(rows)
                y32 = eng.sparse_attention(rp_host, Qd, Kd, Vd, heads=heads, scale=scale, want_y32=True)[2]
                t0 = time.perf_counter()
                leg_one_call()
                first.append((time.perf_counter() - t0) * 1e3)
                first_st = info["bwd"]
                assert first_st["built"] == 1 and first_st["plan_cached"] == 0
                eng.set_option("attn_short", 255)
                leg_one_call()                                # (warm under the other key)
                eng.set_option("attn_short", 256)
                t0 = time.perf_counter()
                leg_one_call()
                replan.append((time.perf_counter() - t0) * 1e3)
                assert info["bwd"]["built"] == 0 and info["bwd"]["plan_cached"] == 0
            legs = [("bwd_one_call", leg_one_call), ("bwd_five_calls_per_head", leg_five_calls),
                    ("fwd_bwd_calls", lambda: fwd_bwd("calls")), ("fwd_bwd_fused", lambda: fwd_bwd("fused"))]
            for _, f in legs:
                f()
            ms = {name: [] for name, _ in legs}
            ev = []
            for _ in range(a.reps):
                for name, f in legs:
                    t0 = time.perf_counter()
                    f()
                    ms[name].append((time.perf_counter() - t0) * 1e3)
                assert info["bwd"]["plan_cached"] == 1
                ev.append(info["bwd"]["attn_ms"])
            st = info["bwd"]
            out = {"tool": "attention_bwd_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "queries": a.queries, "reps": a.reps,
                   "rows": rows if rows == "thresholded" else f"topk{a.topk}", "d": d, "dv": d, "heads": heads, "entries": entries,
                   "segments": int(st["segments"]), "max_row": int(st["max_row"]), "short_rows": int(st["short_rows"]), "long_rows": int(st["long_rows"]),
                   "columns": int(st["columns"]), "max_col": int(st["max_col"]), "short_cols": int(st["short_cols"]), "long_cols": int(st["long_cols"]),
                   "ms": {k: _summary(v) for k, v in ms.items()}, "bwd_kernel_ms": _summary(ev, 4),
                   "first_call_ms": _summary(first), "first_call_transpose_ms": round(first_st["transpose_ms"], 4), "replan_ms": _summary(replan)}
            print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
