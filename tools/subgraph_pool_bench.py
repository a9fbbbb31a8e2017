#!/usr/bin/env python3
"""What max pooling over the induced subgraph of a mini-batch costs through fora_hip_subgraph_pool and fora_hip_subgraph_pool_bwd
against torch.scatter_reduce(..., "amax") and its autograd on the same device.  One JSON line.

  The top --topk rows of --sources sources are put into the row store in calls of --fill sources.  A step is --batch random rows,
  taken, compacted, and the subgraph built; X and G are [nc, d].  Per d in --dims, element type (f32, bf16) and grouping (row,
  col), the legs run alternately --reps times after one warm-up each, and the line carries each leg's median and spread (min,
  max) in ms.

  fwd / fwd_bwd    per value of the option "sub_short" (256: the one-pass kernels take every group of at most 256 entries; 0: every
                   non-empty group takes the long path -- a workgroup of its own forward, segments and the combine backward):
                   call_ms, the C call(s) through ctypes on device tensors made beforehand (a host clock; each call ends in a
                   synchronise); kernel_ms, the calls' own device events (ms_out: the one-pass kernel plus the long path)
  torch            out.scatter_reduce(0, group of e, X[source of e], "amax", include_self=False) in float32, alone and with
                   .backward(G) through autograd (a host clock between two synchronises).  Its backward pass splits the gradient
                   over tied entries; with random normal X there are next to none, so the two sides do the same work

  python tools/subgraph_pool_bench.py --graph webstanford > profiles/subgraph_pool_bench_webstanford.json
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--sources", type=int, default=4000)
    ap.add_argument("--fill", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=64)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--shorts", type=int, nargs="+", default=[256, 0])
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")

    import fora_amd
    from fora_amd import capi, synth
    n, m, row_ptr, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    dev = torch.device("cuda", eng.device)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    default_short = eng.get_option("sub_short")
    rng = np.random.Generator(np.random.PCG64(20261430))
    srcs = synth.query_set(n, a.sources, 20261002)
    R = len(srcs)
    t0 = time.perf_counter()
    for at in range(0, R, a.fill):
        eng.store_put(eng.query_sparse_topk(srcs[at:at + a.fill], a.topk, device=True)[0], append=at > 0)
    fill_s = time.perf_counter() - t0
    lib, ctx = eng._lib, eng._ctx
    info, ms = (ctypes.c_int64 * 4)(), (ctypes.c_double * 3)()

    def forward(X, xtype, flags, out, arg):
        """(call_ms, kernel_ms) of one forward C call on device tensors"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.fora_hip_subgraph_pool(ctx, X.data_ptr(), xtype, X.shape[1], X.stride(0), flags, out.data_ptr(), None, out.stride(0), arg.data_ptr(), arg.stride(0), info, ms)
        dt = (time.perf_counter() - t0) * 1e3
        eng._chk(rc)
        return dt, ms[1] + ms[2]

    def backward(G, flags, arg, out):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.fora_hip_subgraph_pool_bwd(ctx, G.data_ptr(), capi.PROP_F32, G.shape[1], G.stride(0), flags, arg.data_ptr(), arg.stride(0), out.data_ptr(), None, out.stride(0), info, ms)
        dt = (time.perf_counter() - t0) * 1e3
        eng._chk(rc)
        return dt, ms[1] + ms[2]

    def clocked(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    types = {"f32": (torch.float32, capi.PROP_F32), "bf16": (torch.bfloat16, capi.PROP_BF16)}
    bys = {"row": 0, "col": capi.SUB_BY_COL}
    legs = ("fwd", "fwd_bwd")
    res = {f"d{d}_{t}_{by}": {**{leg: {s: {"call_ms": [], "kernel_ms": []} for s in a.shorts} for leg in legs}, "torch": {leg: [] for leg in legs}}
           for d in a.dims for t in types for by in bys}
    ncs, edges, long_rows, long_cols = [], [], [], []
    for step in range(2):                                                    # two mini-batches; every leg alternates inside one
        rows = rng.integers(0, R, size=a.batch)
        _, cols, sub_ptr, sub_col, _, st = eng.store_take_subgraph(rows, device=True)
        nc, E = int(cols.numel()), int(st["edges"])
        ncs.append(nc); edges.append(E)
        in_ptr = eng.subgraph_transpose_fetch(device=True)[0]                # (builds the transposition: no timed call does)
        long_rows.append(int(((sub_ptr[1:] - sub_ptr[:-1]) > 256).sum())); long_cols.append(int(((in_ptr[1:] - in_ptr[:-1]) > 256).sum()))
        ei = capi.subgraph_edge_index(sub_ptr, sub_col)
        ends = {"row": (ei[0].contiguous(), ei[1].contiguous()), "col": (ei[1].contiguous(), ei[0].contiguous())}   # (group, source) of every edge
        for d in a.dims:
            G = torch.randn((nc, d), device=dev)
            for tname, (tdtype, xtype) in types.items():
                X = torch.randn((nc, d), device=dev).to(tdtype)
                out, ref, dx = (torch.empty((nc, d), dtype=torch.float32, device=dev) for _ in range(3))
                arg, aref = (torch.empty((nc, d), dtype=torch.int32, device=dev) for _ in range(2))
                for by, flags in bys.items():
                    r = res[f"d{d}_{tname}_{by}"]
                    index = ends[by][0][:, None].expand(-1, d)
                    source = ends[by][1]

                    def torch_fwd(x):
                        return torch.zeros((nc, d), device=dev).scatter_reduce(0, index, x[source].float(), "amax", include_self=False)

                    def torch_fwd_bwd():
                        x = X.clone().requires_grad_(True)
                        torch_fwd(x).backward(G)
                        return x.grad

                    for rep in range(a.reps + 1):
                        for s in a.shorts:
                            eng.set_option("sub_short", s)
                            first = s == a.shorts[0]
                            dt, k_ms = forward(X, xtype, flags, out if first else ref, arg if first else aref)
                            if rep:
                                r["fwd"][s]["call_ms"].append(dt); r["fwd"][s]["kernel_ms"].append(k_ms)
                            if not first:                                    # the same bits under every value
                                assert torch.equal(out.view(torch.int32), ref.view(torch.int32)) and torch.equal(arg, aref)
                            dt, k_ms = forward(X, xtype, flags, out, arg)
                            dt2, k2_ms = backward(G, flags, arg, dx)
                            if rep:
                                r["fwd_bwd"][s]["call_ms"].append(dt + dt2); r["fwd_bwd"][s]["kernel_ms"].append(k_ms + k2_ms)
                        dt, y = clocked(lambda: torch_fwd(X))
                        dt2, gx = clocked(torch_fwd_bwd)
                        if rep:
                            r["torch"]["fwd"].append(dt); r["torch"]["fwd_bwd"].append(dt2)
                        else:                                                # one look at the values: the same maxima; the same gradient within float32
                            assert torch.equal(y, out), (d, tname, by)       # rounding where autograd adds in float32 (a bfloat16 leaf adds in bfloat16)
                            assert tname != "f32" or torch.allclose(gx, dx, rtol=1e-3, atol=1e-3), (d, tname, by, float((gx - dx).abs().max()))
    eng.set_option("sub_short", default_short)
    out = {"tool": "subgraph_pool_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "reps": a.reps, "steps": 2, "sources": R, "topk": a.topk,
           "fill_s": round(fill_s, 3), "batch": a.batch, "nc": ncs, "edges": edges, "long_rows": long_rows, "long_cols": long_cols}
    for key, r in res.items():
        out[key] = {leg: {str(s): {k: _summary(v) for k, v in r[leg][s].items()} for s in a.shorts} for leg in legs}
        out[key]["torch"] = {leg: _summary(v) for leg, v in r["torch"].items()}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
