#!/usr/bin/env python3
"""What the softmax over each node's edges of a mini-batch's induced subgraph costs through fora_hip_subgraph_softmax and
_softmax_bwd, and a whole attention layer through torch_ops.subgraph_attention, against plain torch on the same device
(DESIGN.md 5.26).  One JSON line.

  The top --topk rows of --sources sources are put into the row store in calls of --fill sources.  A step is --batch random
  rows, taken, compacted, and the subgraph built; scores and g are [heads, edges] float32.  Per head count in --heads and
  grouping (row, col), the legs run alternately --reps times after one warm-up each, and the line carries each leg's median
  and spread (min, max) in ms.

  fwd_ms, bwd_ms    the two C calls through ctypes on device tensors made beforehand (a host clock; a call ends in a synchronise)
  fwd_kernel_ms, bwd_kernel_ms   the calls' own device events (ms_out: the short and the long path added)
  per_head_ms       the forward call as `heads` calls with heads = 1 on the [edges] slices; their bits are compared with the one call's
  torch_ms          torch_ops.row_softmax (scatter operations over repeat_interleave of the offsets) forward and backward on
                    the flattened [heads * edges] scores -- by column after a gather through in_pos -- a host clock between
                    two synchronises; it defines no bits
  attn_ms, attn_torch_ms (by row only, d = --d)   forward and backward of torch_ops.subgraph_attention, and of the same layer
                    in plain torch: gather-multiply-sum scores, row_softmax, index_add aggregation

  python tools/subgraph_softmax_bench.py --graph webstanford
"""
import argparse
import ctypes
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
    rng = np.random.Generator(np.random.PCG64(20261601))
    srcs = synth.query_set(n, a.sources, 20261002)
    R = len(srcs)
    t0 = time.perf_counter()
    for at in range(0, R, a.fill):
        eng.store_put(eng.query_sparse_topk(srcs[at:at + a.fill], a.topk, device=True)[0], append=at > 0)
    fill_s = time.perf_counter() - t0
    lib, ctx = eng._lib, eng._ctx
    info, ms = (ctypes.c_int64 * 4)(), (ctypes.c_double * 2)()

    def fwd(s, heads, flags, out):
        """(call_ms, kernel_ms) of one forward C call on device tensors"""
        dt, rc = _timed(lambda: lib.fora_hip_subgraph_softmax(ctx, s.data_ptr(), capi.PROP_F32, heads, 1.0, flags, out.data_ptr(), None, out.numel(), info, ms))
        eng._chk(rc)
        return dt, ms[0] + ms[1]

    def bwd(y, g, heads, flags, out):
        dt, rc = _timed(lambda: lib.fora_hip_subgraph_softmax_bwd(ctx, y.data_ptr(), capi.PROP_F32, g.data_ptr(), capi.PROP_F32, heads, 1.0, flags,
                                                                 out.data_ptr(), None, out.numel(), info, ms))
        eng._chk(rc)
        return dt, ms[0] + ms[1]

    legs = ("fwd_ms", "fwd_kernel_ms", "bwd_ms", "bwd_kernel_ms", "per_head_ms", "torch_ms")
    res = {f"h{h}_{by}": {k: [] for k in legs} for h in a.heads for by in ("row", "col")}
    attn = {f"h{h}_d{a.d}": {"attn_ms": [], "attn_torch_ms": []} for h in a.heads}
    ncs, edges, longs = [], [], []
    for step in range(2):                                                    # two mini-batches; every leg alternates inside one
        rows = rng.integers(0, R, size=a.batch)
        _, cols, sub_ptr, sub_col, _, st = eng.store_take_subgraph(rows, device=True)
        nc, E = int(cols.numel()), int(st["edges"])
        ncs.append(nc); edges.append(E)
        in_ptr, _, in_pos = eng.subgraph_transpose_fetch(device=True)
        ei = capi.subgraph_edge_index(sub_ptr, sub_col)
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        for heads in a.heads:
            s = torch.randn((heads, E), device=dev) * 4.0
            g = torch.randn((heads, E), device=dev)
            y, one, dx = (torch.empty((heads, E), dtype=torch.float32, device=dev) for _ in range(3))
            for by, flags, ptr in (("row", 0, sub_ptr), ("col", capi.SUB_BY_COL, in_ptr)):
                r = res[f"h{heads}_{by}"]
                # plain torch: every head's groups side by side in one row_ptr of heads * nc groups over the flattened scores
                ptr_all = torch.cat([ptr[:1]] + [ptr[1:] + h * E for h in range(heads)])
                perm = None if by == "row" else torch.cat([in_pos + h * E for h in range(heads)])

                def torch_leg():
                    leaf = s.reshape(-1).clone().requires_grad_(True)
                    yt = torch_ops.row_softmax(ptr_all, leaf if perm is None else leaf[perm])
                    yt.backward(g.reshape(-1) if perm is None else g.reshape(-1)[perm])
                    return yt

                for rep in range(a.reps + 1):
                    t_f, k_f = fwd(s, heads, flags, y)
                    t_heads = sum(fwd(s[h], 1, flags, one[h])[0] for h in range(heads))
                    assert torch.equal(y.view(torch.int32), one.view(torch.int32))          # one call or many: the same bits
                    t_b, k_b = bwd(y, g, heads, flags, dx)
                    t_torch, yt = _timed(torch_leg)
                    if rep:
                        for k, v in zip(legs, (t_f, k_f, t_b, k_b, t_heads, t_torch)):
                            r[k].append(v)
                    else:                                                    # one look at the values: the same softmax within f32 rounding
                        assert torch.allclose(yt.detach(), y.reshape(-1) if perm is None else y.reshape(-1)[perm], rtol=1e-4, atol=1e-6)
                        longs.append(int(info[1]))
            Q, K, V = (torch.randn((nc, heads * a.d), device=dev) for _ in range(3))
            G = torch.randn((nc, heads * a.d), device=dev)
            ptr_all = torch.cat([sub_ptr[:1]] + [sub_ptr[1:] + h * E for h in range(heads)])

            def attn_lib():
                q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
                out = torch_ops.subgraph_attention(eng, q, k, v, heads=heads)
                out.backward(G)
                return out

            def attn_torch():
                q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
                sc = (q[src] * k[dst]).view(E, heads, a.d).sum(-1).t().contiguous() * (a.d ** -0.5)
                yt = torch_ops.row_softmax(ptr_all, sc.reshape(-1)).view(heads, E)
                msg = v[dst].view(E, heads, a.d) * yt.t().unsqueeze(-1)
                out = torch.zeros((nc, heads * a.d), device=dev).index_add(0, src, msg.reshape(E, heads * a.d))
                out.backward(G)
                return out

            for rep in range(a.reps + 1):
                t_lib, o_lib = _timed(attn_lib)
                t_torch, o_torch = _timed(attn_torch)
                if rep:
                    attn[f"h{heads}_d{a.d}"]["attn_ms"].append(t_lib); attn[f"h{heads}_d{a.d}"]["attn_torch_ms"].append(t_torch)
                else:
                    assert torch.allclose(o_lib, o_torch.detach(), rtol=1e-3, atol=1e-3)
    out = {"tool": "subgraph_softmax_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "reps": a.reps, "steps": 2, "sources": R,
           "topk": a.topk, "fill_s": round(fill_s, 3), "batch": a.batch, "nc": ncs, "edges": edges, "long_groups": longs}
    for key, r in list(res.items()) + list(attn.items()):
        out[key] = {k: _summary(v) for k, v in r.items()}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
