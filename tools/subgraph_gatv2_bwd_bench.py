#!/usr/bin/env python3
"""What the backward pass of a GATv2 layer over a mini-batch's induced subgraph costs in ONE library call,
fora_hip_subgraph_gatv2_bwd, against the composed backward pass of torch_ops.subgraph_gatv2 (two library calls, then plain torch
over the edge index head by head), in the same process on the same device tensors.  One JSON line.

  The workload is tools/subgraph_gatv2_bench.py's: the top --topk rows of --sources sources in the row store, a step --batch random
  rows taken, compacted, the subgraph built and transposed; xl, xr [nc, heads * d], att [heads, d], V, G [nc, heads * dv] float32 on
  the device.  Per head count in --heads and grouping (row, col) the legs run alternately --reps times after one warm-up each; the
  line carries each leg's median and spread (min, max) in ms, a host clock between two synchronises around the backward pass alone
  (the forward pass, the same call for both, runs before the clock starts), and for the fused call its own events beside it.

  bwd_fused     out.backward(G) of torch_ops.subgraph_gatv2_trained: one Engine.subgraph_gatv2_bwd call, all four gradients
  bwd_fused_kernel  that call's own device time (short_ms + long_ms)
  bwd_composed  out.backward(G) of torch_ops.subgraph_gatv2

  The warm-up repeat compares the four gradients of the two: equal within float32 rounding.

  python tools/subgraph_gatv2_bwd_bench.py --graph webstanford
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--slope", type=float, default=0.2)
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
    rng = np.random.Generator(np.random.PCG64(20261801))
    srcs = synth.query_set(n, a.sources, 20261002)
    R = len(srcs)
    for at in range(0, R, a.fill):
        eng.store_put(eng.query_sparse_topk(srcs[at:at + a.fill], a.topk, device=True)[0], append=at > 0)

    legs = ("bwd_fused_ms", "bwd_fused_kernel_ms", "bwd_composed_ms")
    res = {f"h{h}_{by}": {k: [] for k in legs} for h in a.heads for by in ("row", "col")}
    ncs, edges, longs = [], [], []
    for step in range(2):                                                    # two mini-batches; the legs alternate inside one
        rows = rng.integers(0, R, size=a.batch)
        _, cols, _, _, _, st = eng.store_take_subgraph(rows, device=True)
        nc = int(cols.numel())
        ncs.append(nc); edges.append(int(st["edges"]))
        eng.subgraph_transpose_fetch(device=True)                            # (built here: no leg pays for it)
        for heads in a.heads:
            xl, xr = (torch.randn((nc, heads * a.d), device=dev) for _ in range(2))
            att = torch.randn((heads, a.d), device=dev)
            V, G = (torch.randn((nc, heads * a.dv), device=dev) for _ in range(2))
            for by, direction in (("row", "out"), ("col", "in")):
                r = res[f"h{heads}_{by}"]

                def backward(fn):
                    leaves = [x.clone().requires_grad_(True) for x in (xl, xr, att, V)]
                    out = fn(eng, *leaves, heads=heads, slope=a.slope, direction=direction)
                    ms, _ = _timed(lambda: out.backward(G))
                    return ms, [x.grad for x in leaves]

                for rep in range(a.reps + 1):
                    t_f, g_f = backward(torch_ops.subgraph_gatv2_trained)
                    st_f = eng.last_subgraph_gatv2_bwd
                    t_c, g_c = backward(torch_ops.subgraph_gatv2)
                    if rep:
                        for k, v in zip(legs, (t_f, st_f["short_ms"] + st_f["long_ms"], t_c)):
                            r[k].append(v)
                    else:                                                    # one look at the values
                        assert all(torch.allclose(x, z, rtol=1e-3, atol=1e-3) for x, z in zip(g_f, g_c))
                        longs.append([st_f["long_groups"], st_f["across_long"]])
    out = {"tool": "subgraph_gatv2_bwd_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "reps": a.reps, "steps": 2, "sources": R,
           "topk": a.topk, "batch": a.batch, "d": a.d, "dv": a.dv, "slope": a.slope, "nc": ncs, "edges": edges, "long_groups": longs}
    for key, r in res.items():
        out[key] = {k: _summary(v) for k, v in r.items()}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
