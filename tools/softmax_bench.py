#!/usr/bin/env python3
"""What the row softmax on the held pattern costs: one held sparse result of --queries sources -- the full
thresholded rows (threshold 1 / n) and the rows cut to their --topk largest entries -- device resident float32 scores and
gradient [entries], and the legs

  (a) sparse_softmax                                   the forward call
  (b) sparse_softmax_bwd                               the backward call on (a)'s float32 output
  (c) torch row_softmax, forward                       fora_amd.torch_ops.row_softmax: repeat_interleave, scatter_reduce, index_add, gathers
  (d) torch row_softmax, forward + backward            ... and autograd through it: the yardstick of (a) + (b)
  (e) ppr_attention(softmax="torch"), forward + backward   Q [nq, d], K [n, d], V [n, d], end to end
  (f) ppr_attention(softmax="engine"), forward + backward

Every leg is warmed up once; then the legs run alternately --reps times and the line carries each leg's median and spread
(min, max) in ms per call.  Times are a host clock around calls that end in a synchronise; fwd_kernel_ms / bwd_kernel_ms are
the library's device events.

  python tools/softmax_bench.py --graph webstanford
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
    ap.add_argument("--scale", type=float, default=0.125)
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")

    import fora_amd
    from fora_amd import synth
    from fora_amd.torch_ops import ppr_attention, row_softmax
    n, m, row_ptr, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    dev = torch.device("cuda", eng.device)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    srcs = synth.query_set(n, a.queries, 20261001)
    nq = len(srcs)
    rng = np.random.Generator(np.random.PCG64(20261019))
    d = a.d
    Q = torch.from_numpy(rng.standard_normal((nq, d), dtype=np.float32)).to(dev).requires_grad_(True)
    K = torch.from_numpy(rng.standard_normal((n, d), dtype=np.float32)).to(dev).requires_grad_(True)
    V = torch.from_numpy(rng.standard_normal((n, d), dtype=np.float32)).to(dev).requires_grad_(True)
    G = torch.from_numpy(rng.standard_normal((nq, d), dtype=np.float32)).to(dev)

    for rows in ("thresholded", f"topk{a.topk}"):
        if rows == "thresholded":
            rp = eng.query_sparse(srcs, device=True)[0]
        else:
            rp = eng.query_sparse_topk(srcs, a.topk, device=True)[0]
        torch.cuda.synchronize()
        rp_host = rp.cpu().numpy()
        entries = int(rp_host[-1])
        scores = torch.from_numpy(rng.standard_normal(entries, dtype=np.float32) * 8).to(dev)
        grad = torch.from_numpy(rng.standard_normal(entries, dtype=np.float32)).to(dev)
        info = {}

        def leg_fwd():
            info["y"], _, info["fwd"] = eng.sparse_softmax(rp_host, scores, scale=a.scale)

        def leg_bwd():
            _, _, info["bwd"] = eng.sparse_softmax_bwd(rp_host, info["y"], grad, scale=a.scale)

        def leg_torch_fwd():
            with torch.no_grad():
                row_softmax(rp, scores * a.scale)
            torch.cuda.synchronize()

        def leg_torch_fwd_bwd():
            s = scores.detach().requires_grad_(True)
            row_softmax(rp, s * a.scale).backward(grad)
            torch.cuda.synchronize()

        def attention(softmax):
            def leg():
                for x in (Q, K, V):
                    x.grad = None
                ppr_attention(eng, rp_host, Q, K, V, softmax=softmax).backward(G)
                torch.cuda.synchronize()
            return leg

        legs = [("softmax_fwd", leg_fwd), ("softmax_bwd", leg_bwd), ("torch_row_softmax_fwd", leg_torch_fwd),
                ("torch_row_softmax_fwd_bwd", leg_torch_fwd_bwd), ("attention_torch_softmax", attention("torch")),
                ("attention_engine_softmax", attention("engine"))]
        for _, f in legs:
            f()
        ms = {name: [] for name, _ in legs}
        ev = {"fwd_kernel": [], "bwd_kernel": []}
        for _ in range(a.reps):
            for name, f in legs:
                t0 = time.perf_counter()
                f()
                ms[name].append((time.perf_counter() - t0) * 1e3)
            ev["fwd_kernel"].append(info["fwd"]["softmax_ms"])
            ev["bwd_kernel"].append(info["bwd"]["softmax_ms"])
        ms["softmax_fwd_bwd"] = [x + y for x, y in zip(ms["softmax_fwd"], ms["softmax_bwd"])]
        st = info["fwd"]
        out = {"tool": "softmax_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "queries": a.queries, "reps": a.reps,
               "rows": rows, "d": d, "scale": a.scale, "entries": entries, "segments": int(st["segments"]), "max_row": int(st["max_row"]),
               "short_rows": int(st["short_rows"]), "long_rows": int(st["long_rows"]), "nan_rows": int(st["nan_rows"]),
               "ms": {k: _summary(v) for k, v in ms.items()},
               "fwd_kernel_ms": _summary(ev["fwd_kernel"], 4), "bwd_kernel_ms": _summary(ev["bwd_kernel"], 4)}
        print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
