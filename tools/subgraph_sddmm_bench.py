#!/usr/bin/env python3
"""What the scores of every edge of a mini-batch's induced subgraph cost through fora_hip_subgraph_sddmm against the same
scores head by head and against plain torch on the same device.  One JSON line.

  The top --topk rows of --sources sources are put into the row store in calls of --fill sources.  A step is --batch random
  rows, taken, compacted, and the subgraph built; A and B are [nc, heads * d].  Per case heads x d in --cases and element type
  (f32, bf16), the legs run alternately --reps times after one warm-up each, and the line carries each leg's median and
  spread (min, max) in ms.

  call_ms      the C call through ctypes on device tensors made beforehand (a host clock; the call ends in a synchronise)
  kernel_ms    the call's own device event (ms_out: k_sub_sddmm)
  per_head_ms  the same scores as `heads` calls with heads = 1 on column slices (a host clock around all of them); their bits
               are compared with the one call's
  torch_ms     (A[row of e] * B[col of e]).view(E, heads, d).sum(-1) in float32 (a host clock between two synchronises); it
               materialises two [E, heads * d] matrices and defines no bits
  torch.sparse legs are left out.

  python tools/subgraph_sddmm_bench.py --graph webstanford
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
    ap.add_argument("--cases", nargs="+", default=["1x64", "8x16", "8x64"], help="heads x d")
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")
    cases = [tuple(int(x) for x in c.split("x")) for c in a.cases]

    import fora_amd
    from fora_amd import capi, synth
    n, m, row_ptr, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    dev = torch.device("cuda", eng.device)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    rng = np.random.Generator(np.random.PCG64(20261501))
    srcs = synth.query_set(n, a.sources, 20261002)
    R = len(srcs)
    t0 = time.perf_counter()
    for at in range(0, R, a.fill):
        eng.store_put(eng.query_sparse_topk(srcs[at:at + a.fill], a.topk, device=True)[0], append=at > 0)
    fill_s = time.perf_counter() - t0
    fn, ctx = eng._lib.fora_hip_subgraph_sddmm, eng._ctx
    info, ms = (ctypes.c_int64 * 4)(), ctypes.c_double(0)

    def call(A, B, xtype, d, heads, out):
        """(call_ms, kernel_ms) of one C call on device tensors; A and B may be column slices"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = fn(ctx, A.data_ptr(), xtype, A.stride(0), B.data_ptr(), xtype, B.stride(0), d, heads, out.data_ptr(), None, out.numel(), info, ctypes.byref(ms))
        dt = (time.perf_counter() - t0) * 1e3
        eng._chk(rc)
        return dt, ms.value

    types = {"f32": (torch.float32, capi.PROP_F32), "bf16": (torch.bfloat16, capi.PROP_BF16)}
    res = {f"h{h}_d{d}_{t}": {"call_ms": [], "kernel_ms": [], "per_head_ms": [], "torch_ms": []} for h, d in cases for t in types}
    ncs, edges = [], []
    for step in range(2):                                                    # two mini-batches; every leg alternates inside one
        rows = rng.integers(0, R, size=a.batch)
        _, cols, sub_ptr, sub_col, _, st = eng.store_take_subgraph(rows, device=True)
        nc, E = int(cols.numel()), int(st["edges"])
        ncs.append(nc); edges.append(E)
        ei = capi.subgraph_edge_index(sub_ptr, sub_col)
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        for heads, d in cases:
            for tname, (tdtype, xtype) in types.items():
                r = res[f"h{heads}_d{d}_{tname}"]
                A = torch.randn((nc, heads * d), device=dev).to(tdtype)
                B = torch.randn((nc, heads * d), device=dev).to(tdtype)
                out = torch.empty((heads, E), dtype=torch.float32, device=dev)
                ref = torch.empty((heads, E), dtype=torch.float32, device=dev)
                torch.cuda.synchronize()
                for rep in range(a.reps + 1):
                    dt, k_ms = call(A, B, xtype, d, heads, out)
                    t_heads = 0.0
                    for h in range(heads):
                        t_heads += call(A[:, h * d:(h + 1) * d], B[:, h * d:(h + 1) * d], xtype, d, 1, ref[h])[0]
                    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))     # one call or many: the same bits
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    y = (A[src].float() * B[dst].float()).view(E, heads, d).sum(-1)
                    torch.cuda.synchronize()
                    t_torch = (time.perf_counter() - t0) * 1e3
                    if rep:
                        r["call_ms"].append(dt); r["kernel_ms"].append(k_ms); r["per_head_ms"].append(t_heads); r["torch_ms"].append(t_torch)
                    else:                                                    # one look at the values: the same scores within f32 rounding
                        assert torch.allclose(y.t(), out, rtol=1e-3, atol=1e-3)
    out = {"tool": "subgraph_sddmm_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "reps": a.reps, "steps": 2, "sources": R,
           "topk": a.topk, "fill_s": round(fill_s, 3), "batch": a.batch, "nc": ncs, "edges": edges}
    for key, r in res.items():
        out[key] = {k: _summary(v) for k, v in r.items()}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
