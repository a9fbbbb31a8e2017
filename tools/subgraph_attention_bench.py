#!/usr/bin/env python3
"""What an attention layer over a mini-batch's induced subgraph costs in ONE call, fora_hip_subgraph_attention, against the same
work as the chain of calls it replaces, in the same process on the same device tensors.  One JSON line.

  The top --topk rows of --sources sources are put into the row store in calls of --fill sources.  A step is --batch random
  rows, taken, compacted, and the subgraph built; Q, K are [nc, heads * d] and V is [nc, heads * dv] float32 on the device.  Per
  head count in --heads and grouping (row, col), the legs run alternately --reps times after one warm-up each, and the line
  carries each leg's median and spread (min, max) in ms.

  fused_ms, fused_kernel_ms     Engine.subgraph_attention with a caller-made out32 and y32 wanted (what a training step keeps): a
                                host clock between two synchronises, and the call's own device events (short and long path added)
  fused_noy_ms                  the same call without y (inference)
  chain_ms, chain_kernel_ms     subgraph_sddmm + subgraph_softmax + `heads` x subgraph_propagate(values=y[h]) (propagate_t by
                                column) into the column slices of a caller-made out32: the host clock, and the calls' events added
  layer_fused_ms, layer_chain_ms   forward and backward of torch_ops.subgraph_attention_fused and of torch_ops.subgraph_attention

  The warm-up repeat compares the two forward results: equal within float32 rounding of the probabilities (the chain rounds
  scores and probabilities to float32 between its steps, the one call does not).

  python tools/subgraph_attention_bench.py --graph webstanford
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


def _summary(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def _timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--sources", type=int, default=4000)
    ap.add_argument("--fill", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=64)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--heads", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--dv", type=int, default=16)
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")

    import fora_amd
    from fora_amd import synth, torch_ops
    n, m, row_ptr, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    dev = torch.device("cuda", eng.device)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    rng = np.random.Generator(np.random.PCG64(20261701))
    srcs = synth.query_set(n, a.sources, 20261002)
    R = len(srcs)
    t0 = time.perf_counter()
    for at in range(0, R, a.fill):
        eng.store_put(eng.query_sparse_topk(srcs[at:at + a.fill], a.topk, device=True)[0], append=at > 0)
    fill_s = time.perf_counter() - t0
    scale = a.d ** -0.5

    legs = ("fused_ms", "fused_kernel_ms", "fused_noy_ms", "chain_ms", "chain_kernel_ms", "layer_fused_ms", "layer_chain_ms")
    res = {f"h{h}_{by}": {k: [] for k in legs} for h in a.heads for by in ("row", "col")}
    ncs, edges, longs = [], [], []
    for step in range(2):                                                    # two mini-batches; every leg alternates inside one
        rows = rng.integers(0, R, size=a.batch)
        _, cols, _, _, _, st = eng.store_take_subgraph(rows, device=True)
        nc, E = int(cols.numel()), int(st["edges"])
        ncs.append(nc); edges.append(E)
        eng.subgraph_transpose_fetch(device=True)                            # (built here: no leg pays for it)
        for heads in a.heads:
            Q, K = (torch.randn((nc, heads * a.d), device=dev) for _ in range(2))
            V, G = (torch.randn((nc, heads * a.dv), device=dev) for _ in range(2))
            o_fused, o_chain = (torch.empty((nc, heads * a.dv), dtype=torch.float32, device=dev) for _ in range(2))
            sc, y = (torch.empty((heads, E), dtype=torch.float32, device=dev) for _ in range(2))
            for by, direction in (("row", "out"), ("col", "in")):
                r = res[f"h{heads}_{by}"]
                product = eng.subgraph_propagate if by == "row" else eng.subgraph_propagate_t

                def fused(want_y):
                    return eng.subgraph_attention(Q, K, V, heads=heads, scale=scale, by=by, want_y32=want_y, out32=o_fused)[4]

                def chain():
                    kernel = eng.subgraph_sddmm(*((Q, K) if by == "row" else (K, Q)), heads=heads, out32=sc)[2]["sddmm_ms"]
                    s = eng.subgraph_softmax(sc, scale=scale, by=by, out32=y)[2]
                    kernel += s["short_ms"] + s["long_ms"]
                    for h in range(heads):
                        vs = slice(h * a.dv, (h + 1) * a.dv)
                        p = product(V[:, vs], values=y[h], want64=False, out32=o_chain[:, vs])[2]
                        kernel += p["transpose_ms"] + p["short_ms"] + p["long_ms"]
                    return kernel

                def layer(fn):
                    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
                    fn(eng, q, k, v, heads=heads, direction=direction).backward(G)

                for rep in range(a.reps + 1):
                    t_f, st_f = _timed(lambda: fused(True))
                    t_n, _ = _timed(lambda: fused(False))
                    t_c, k_c = _timed(chain)
                    t_lf, _ = _timed(lambda: layer(torch_ops.subgraph_attention_fused))
                    t_lc, _ = _timed(lambda: layer(torch_ops.subgraph_attention))
                    if rep:
                        for k, v in zip(legs, (t_f, st_f["short_ms"] + st_f["long_ms"], t_n, t_c, k_c, t_lf, t_lc)):
                            r[k].append(v)
                    else:                                                    # one look at the values
                        assert torch.allclose(o_fused, o_chain, rtol=1e-4, atol=1e-5)
                        longs.append(st_f["long_groups"])
    out = {"tool": "subgraph_attention_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "reps": a.reps, "steps": 2, "sources": R,
           "topk": a.topk, "fill_s": round(fill_s, 3), "batch": a.batch, "d": a.d, "dv": a.dv, "nc": ncs, "edges": edges, "long_groups": longs}
    for key, r in res.items():
        out[key] = {k: _summary(v) for k, v in r.items()}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
