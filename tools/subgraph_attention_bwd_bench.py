#!/usr/bin/env python3
"""What the backward pass of an attention layer over a mini-batch's induced subgraph costs in ONE call,
fora_hip_subgraph_attention_bwd, against the chain of calls it replaces, in the same process on the same device tensors and the
same saved y32.  One JSON line.

  The workload is tools/subgraph_attention_bench.py's: the top --topk rows of --sources sources in the row store, a step --batch
  random rows taken, compacted, the subgraph built and transposed; Q, K [nc, heads * d], V, G [nc, heads * dv] float32 on the
  device.  Per head count in --heads and grouping (row, col) the legs run alternately --reps times after one warm-up each; the
  line carries each leg's median and spread (min, max) in ms.

  bwd_ms, bwd_kernel_ms     Engine.subgraph_attention_bwd with caller-made dq32, dk32, dv32: a host clock between two
                            synchronises, and the call's own device events (fused kernels and the longer groups' path added)
  chain_ms, chain_kernel_ms the 2 + 3 * heads calls torch_ops.subgraph_attention_fused's backward pass makes -- `heads` across
                            products for dv, subgraph_sddmm, subgraph_softmax_bwd, `heads` along and `heads` across products --
                            into the column slices of caller-made outputs: the host clock, and the calls' events added
  layer_trained_ms, layer_fused_ms   forward and backward of torch_ops.subgraph_attention_trained and of subgraph_attention_fused

  The warm-up repeat compares the two results: equal within float32 rounding of dy and ds (the chain rounds both to float32
  between its steps, the one call does not).

  python tools/subgraph_attention_bwd_bench.py --graph webstanford
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # before the library is loaded: one HIP runtime in the process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from subgraph_attention_bench import _summary, _timed  # noqa: E402


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
    for at in range(0, R, a.fill):
        eng.store_put(eng.query_sparse_topk(srcs[at:at + a.fill], a.topk, device=True)[0], append=at > 0)
    scale = a.d ** -0.5

    legs = ("bwd_ms", "bwd_kernel_ms", "chain_ms", "chain_kernel_ms", "layer_trained_ms", "layer_fused_ms")
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
            new = lambda X: torch.empty(X.shape, dtype=torch.float32, device=dev)
            one, chn = [new(X) for X in (Q, K, V)], [new(X) for X in (Q, K, V)]
            for by, direction in (("row", "out"), ("col", "in")):
                r = res[f"h{heads}_{by}"]
                y32 = eng.subgraph_attention(Q, K, V, heads=heads, scale=scale, by=by, want_y32=True)[2]
                along, across = (eng.subgraph_propagate, eng.subgraph_propagate_t) if by == "row" else (eng.subgraph_propagate_t, eng.subgraph_propagate)

                def bwd():
                    return eng.subgraph_attention_bwd(Q, K, V, G, y32, heads=heads, scale=scale, by=by, dq32=one[0], dk32=one[1], dv32=one[2])[6]

                def chain():
                    ms = lambda p: p["transpose_ms"] + p["short_ms"] + p["long_ms"]
                    kernel = 0.0
                    for h in range(heads):
                        vs = slice(h * a.dv, (h + 1) * a.dv)
                        kernel += ms(across(G[:, vs], values=y32[h], want64=False, out32=chn[2][:, vs])[2])
                    dy, _, s = eng.subgraph_sddmm(*((G, V) if by == "row" else (V, G)), heads=heads)
                    ds, _, b = eng.subgraph_softmax_bwd(y32, dy, scale=scale, by=by)
                    kernel += s["sddmm_ms"] + b["short_ms"] + b["long_ms"]
                    for h in range(heads):
                        qs = slice(h * a.d, (h + 1) * a.d)
                        kernel += ms(along(K[:, qs], values=ds[h], want64=False, out32=chn[0][:, qs])[2])
                        kernel += ms(across(Q[:, qs], values=ds[h], want64=False, out32=chn[1][:, qs])[2])
                    return kernel

                def layer(fn):
                    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
                    fn(eng, q, k, v, heads=heads, direction=direction).backward(G)

                for rep in range(a.reps + 1):
                    t_b, st_b = _timed(bwd)
                    t_c, k_c = _timed(chain)
                    t_lt, _ = _timed(lambda: layer(torch_ops.subgraph_attention_trained))
                    t_lf, _ = _timed(lambda: layer(torch_ops.subgraph_attention_fused))
                    if rep:
                        for k, v in zip(legs, (t_b, st_b["short_ms"] + st_b["long_ms"], t_c, k_c, t_lt, t_lf)):
                            r[k].append(v)
                    else:                                                    # one look at the values
                        assert all(torch.allclose(x, z, rtol=1e-3, atol=1e-4) for x, z in zip(one, chn))
                        longs.append([st_b["long_groups"], st_b["across_long"]])
    out = {"tool": "subgraph_attention_bwd_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "reps": a.reps, "steps": 2, "sources": R,
           "topk": a.topk, "batch": a.batch, "d": a.d, "dv": a.dv, "nc": ncs, "edges": edges, "long_groups": longs}
    for key, r in res.items():
        out[key] = {k: _summary(v) for k, v in r.items()}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
