#!/usr/bin/env python3
"""What a GATv2 layer over a mini-batch's induced subgraph costs with the library's fused forward call, fora_hip_subgraph_gatv2,
against what a user has without it, in the same process on the same device tensors.  One JSON line.

  The workload is tools/subgraph_gat_bench.py's: the top --topk rows of --sources sources in the row store, a step --batch random
  rows taken, compacted, the subgraph built and transposed; xl, xr [nc, heads * d], att [heads, d], V, G [nc, heads * dv] float32 on
  the device.  Per head count in --heads and grouping (row, col) the legs run alternately --reps times after one warm-up each; the
  line carries each leg's median and spread (min, max) in ms: a host clock between two synchronises, and beside it device time --
  the call's own events for the library's forward (fwd_gatv2_kernel_ms), torch.cuda events around the plain-torch legs (*_event_ms).

  fwd_gatv2    Engine.subgraph_gatv2 with a caller-made out32 and y32
  fwd_torch    the plain-torch expression: two gathers over all edges, add, leaky_relu, multiply-sum with att, a scatter softmax,
               index_add_ -- [edges, heads * d] materialised
  layer_*      forward and backward of the two through autograd (gatv2: torch_ops.subgraph_gatv2, whose backward pass composes
               the existing calls and plain torch)

  The warm-up repeat compares the two outputs and the four gradients: equal within float32 rounding.

  python tools/subgraph_gatv2_bench.py --graph webstanford
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
from subgraph_gat_bench import _evented  # noqa: E402


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
    from fora_amd import capi, synth, torch_ops
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

    legs = ("fwd_gatv2_ms", "fwd_gatv2_kernel_ms", "fwd_torch_ms", "fwd_torch_event_ms", "layer_gatv2_ms", "layer_torch_ms", "layer_torch_event_ms")
    res = {f"h{h}_{by}": {k: [] for k in legs} for h in a.heads for by in ("row", "col")}
    ncs, edges, longs = [], [], []
    for step in range(2):                                                    # two mini-batches; every leg alternates inside one
        rows = rng.integers(0, R, size=a.batch)
        _, cols, sub_ptr, sub_col, _, st = eng.store_take_subgraph(rows, device=True)
        nc, E = int(cols.numel()), int(st["edges"])
        ncs.append(nc); edges.append(E)
        eng.subgraph_transpose_fetch(device=True)                            # (built here: no leg pays for it)
        src, dst = capi.subgraph_edge_index(sub_ptr, sub_col)
        for heads in a.heads:
            xl, xr = (torch.randn((nc, heads * a.d), device=dev) for _ in range(2))
            att = torch.randn((heads, a.d), device=dev)
            V, G = (torch.randn((nc, heads * a.dv), device=dev) for _ in range(2))
            out32 = torch.empty_like(V)
            for by, direction in (("row", "out"), ("col", "in")):
                r = res[f"h{heads}_{by}"]
                grp, oth = (src, dst) if by == "row" else (dst, src)

                def gatv2(l, rr, aa, v):
                    return torch_ops.subgraph_gatv2(eng, l, rr, aa, v, heads=heads, slope=a.slope, direction=direction)

                def plain(l, rr, aa, v):
                    s = (aa * torch.nn.functional.leaky_relu((l[src] + rr[dst]).view(-1, heads, a.d), a.slope)).sum(-1)    # [E, heads]
                    mx = torch.full((nc, heads), -torch.inf, device=dev).scatter_reduce(0, grp[:, None].expand(-1, heads), s.detach(), "amax")
                    p = torch.exp(s - mx[grp])
                    y = p / torch.zeros((nc, heads), device=dev).index_add_(0, grp, p)[grp]
                    return torch.zeros((nc, heads, a.dv), device=dev).index_add_(0, grp, y[:, :, None] * v.view(nc, heads, a.dv)[oth]).view(nc, heads * a.dv)

                def layer(fn):
                    leaves = [x.clone().requires_grad_(True) for x in (xl, xr, att, V)]
                    fn(*leaves).backward(G)
                    return [x.grad for x in leaves]

                def fwd(fn):
                    with torch.no_grad():
                        return fn(xl, xr, att, V)

                for rep in range(a.reps + 1):
                    t_g, st_g = _timed(lambda: eng.subgraph_gatv2(xl, xr, att, V, heads=heads, slope=a.slope, by=by, out32=out32, want_y32=True)[4])
                    t_t, e_t, o_t = _evented(lambda: fwd(plain))
                    t_lg, g_g = _timed(lambda: layer(gatv2))
                    t_lt, e_lt, g_t = _evented(lambda: layer(plain))
                    if rep:
                        for k, v in zip(legs, (t_g, st_g["short_ms"] + st_g["long_ms"], t_t, e_t, t_lg, t_lt, e_lt)):
                            r[k].append(v)
                    else:                                                    # one look at the values
                        assert torch.allclose(out32, o_t, rtol=1e-3, atol=1e-4)
                        assert all(torch.allclose(x, z, rtol=1e-3, atol=1e-3) for x, z in zip(g_g, g_t))
                        longs.append(st_g["long_groups"])
    out = {"tool": "subgraph_gatv2_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "reps": a.reps, "steps": 2, "sources": R,
           "topk": a.topk, "batch": a.batch, "d": a.d, "dv": a.dv, "slope": a.slope, "nc": ncs, "edges": edges, "long_groups": longs}
    for key, r in res.items():
        out[key] = {k: _summary(v) for k, v in r.items()}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
