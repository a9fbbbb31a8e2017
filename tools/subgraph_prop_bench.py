#!/usr/bin/env python3
"""What one message-passing step over the induced subgraph of a mini-batch costs through fora_hip_subgraph_propagate and
fora_hip_subgraph_propagate_t against plain torch on the same device.  One JSON line.

  The top --topk rows of --sources sources are put into the row store in calls of --fill sources.  A step is --batch random
  rows, taken, compacted, and the subgraph built; X is [nc, d].  Per d in --dims and element type (f32, bf16), the legs run
  alternately --reps times after one warm-up each, and the line carries each leg's median and spread (min, max) in ms.

  forward / transposed   per value of the option "sub_short" (256: the one-pass kernel k_sub_agg takes every row of at most 256
                         entries; 0: every row goes through the gather and combine kernels of PROPAGATE): call_ms, the C call
                         through ctypes on device tensors made beforehand (a host clock; the call ends in a synchronise);
                         kernel_ms, the call's own device events (ms_out: the one-pass kernel plus the long path);
                         first_t_ms, the first transposed call of a step, which builds the transposition, and its
                         transpose_ms
  torch_scatter          out.index_add_(0, row of e, X[col of e]) and the reverse, float32 accumulation (a host clock between
                         two synchronises)
  torch.sparse.mm over a CSR made from the fetched arrays is NOT a leg: with the torch and ROCm this tool was first run on,
  the first such product ended the process from inside hipSPARSE (an uncaught C++ exception of type `char const*`), which no
  Python code can catch

  python tools/subgraph_prop_bench.py --graph webstanford
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
    rng = np.random.Generator(np.random.PCG64(20261401))
    srcs = synth.query_set(n, a.sources, 20261002)
    R = len(srcs)
    t0 = time.perf_counter()
    for at in range(0, R, a.fill):
        eng.store_put(eng.query_sparse_topk(srcs[at:at + a.fill], a.topk, device=True)[0], append=at > 0)
    fill_s = time.perf_counter() - t0
    lib, ctx = eng._lib, eng._ctx
    info, ms = (ctypes.c_int64 * 4)(), (ctypes.c_double * 3)()

    def call(fn, X, xtype, out):
        """(call_ms, kernel_ms, transpose_ms, built) of one C call on device tensors"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = fn(ctx, X.data_ptr(), xtype, X.shape[1], X.stride(0), 0, None, 0, out.data_ptr(), None, out.stride(0), info, ms)
        dt = (time.perf_counter() - t0) * 1e3
        eng._chk(rc)
        return dt, ms[1] + ms[2], ms[0], int(info[0])

    def clocked(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    types = {"f32": (torch.float32, capi.PROP_F32), "bf16": (torch.bfloat16, capi.PROP_BF16)}
    res = {f"d{d}_{t}": {"forward": {s: {"call_ms": [], "kernel_ms": []} for s in a.shorts},
                         "transposed": {s: {"call_ms": [], "kernel_ms": []} for s in a.shorts},
                         "torch_scatter": {"forward": [], "transposed": []}}
           for d in a.dims for t in types}
    first_t, first_tr, ncs, edges, long_rows, long_cols = [], [], [], [], [], []
    for step in range(2):                                                    # two mini-batches; every leg alternates inside one
        rows = rng.integers(0, R, size=a.batch)
        _, cols, sub_ptr, sub_col, _, st = eng.store_take_subgraph(rows, device=True)
        nc, E = int(cols.numel()), int(st["edges"])
        ncs.append(nc); edges.append(E)
        in_ptr, in_row, in_pos = None, None, None
        ei = capi.subgraph_edge_index(sub_ptr, sub_col)
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        for d in a.dims:
            for tname, (tdtype, xtype) in types.items():
                r = res[f"d{d}_{tname}"]
                X = torch.randn((nc, d), device=dev).to(tdtype)
                out = torch.empty((nc, d), dtype=torch.float32, device=dev)
                ref = torch.empty((nc, d), dtype=torch.float32, device=dev)
                if in_ptr is None:                                           # the first transposed call of the step builds the transposition
                    dt, _, tr_ms, built = call(lib.fora_hip_subgraph_propagate_t, X, xtype, out)
                    assert built == 1
                    first_t.append(dt); first_tr.append(tr_ms)
                    in_ptr, in_row, in_pos = eng.subgraph_transpose_fetch(device=True)
                    long_rows.append(int(((sub_ptr[1:] - sub_ptr[:-1]) > 256).sum())); long_cols.append(int(((in_ptr[1:] - in_ptr[:-1]) > 256).sum()))
                torch.cuda.synchronize()
                for rep in range(a.reps + 1):
                    for s in a.shorts:
                        eng.set_option("sub_short", s)
                        for side, fn in (("forward", lib.fora_hip_subgraph_propagate), ("transposed", lib.fora_hip_subgraph_propagate_t)):
                            dt, k_ms, _, built = call(fn, X, xtype, out if s == a.shorts[0] else ref)
                            assert built == 0
                            if rep:
                                r[side][s]["call_ms"].append(dt); r[side][s]["kernel_ms"].append(k_ms)
                        if s != a.shorts[0]:
                            assert torch.equal(out.view(torch.int32), ref.view(torch.int32))  # the same bits under every value (the transposed call's here)
                    legs = (("torch_scatter", "forward", lambda: torch.zeros((nc, d), device=dev).index_add_(0, src, X[dst].float())),
                            ("torch_scatter", "transposed", lambda: torch.zeros((nc, d), device=dev).index_add_(0, dst, X[src].float())))
                    for leg, side, f in legs:
                        dt, y = clocked(f)
                        if rep:
                            r[leg][side].append(dt)
                        elif side == "transposed":                           # one look at the values: the same product within f32 rounding
                            assert torch.allclose(y, out, rtol=1e-3, atol=1e-3)
    eng.set_option("sub_short", default_short)
    out = {"tool": "subgraph_prop_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "reps": a.reps, "steps": 2, "sources": R,
           "topk": a.topk, "fill_s": round(fill_s, 3), "batch": a.batch, "nc": ncs, "edges": edges, "long_rows": long_rows, "long_cols": long_cols,
           "first_t_ms": _summary(first_t), "first_transpose_ms": _summary(first_tr)}
    for key, r in res.items():
        out[key] = {side: {str(s): {k: _summary(v) for k, v in r[side][s].items()} for s in a.shorts} for side in ("forward", "transposed")}
        out[key]["torch_scatter"] = {side: _summary(v) for side, v in r["torch_scatter"].items()}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
