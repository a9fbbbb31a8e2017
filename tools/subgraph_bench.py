#!/usr/bin/env python3
"""What the induced subgraph of a mini-batch of stored PPR rows costs through fora_hip_sparse_subgraph against plain torch on
the same device.  One JSON line.

  The top --topk rows of --sources sources are put into the row store in calls of --fill sources.  A step is --batch random
  rows, taken and compacted; U is the step's columns.  The library has no earlier call for this, so the comparison is torch in
  the same run; legs run alternately --reps times after one warm-up each, and the line carries each leg's median and spread
  (min, max) in ms -- a host clock around calls that end in a synchronise unless named a kernel time, which are the library's
  device events.

  nc, scanned, edges   the columns of the steps' batches, the out-degrees of U added up, the edges kept
  subgraph             per call under every --spans value of the option "sub_span": call_ms, fora_hip_sparse_subgraph alone (the C
                       call through ctypes, nothing fetched); binding_ms, Engine.sparse_subgraph(device=True, want_eid=True) (that
                       call, three device tensors, a device synchronise and the fetch); kernel_ms, the call's ms_out
  torch_mask           mask[src] & mask[dst] over all m edges, the kept pairs relabelled through an inverse map
  torch_rows           the rows of U gathered (repeat_interleave over their degrees), torch.isin against U, the same relabelling

  python tools/subgraph_bench.py --graph webstanford
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


def _summary(v, digits=3):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--sources", type=int, default=20000)
    ap.add_argument("--fill", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=64)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spans", type=int, nargs="+", default=[1024, 2048, 4096])
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")

    import fora_amd
    from fora_amd import synth
    n, m, row_ptr, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    dev = torch.device("cuda", eng.device)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    default_span = eng.get_option("sub_span")
    rng = np.random.Generator(np.random.PCG64(20261301))
    srcs = synth.query_set(n, a.sources, 20261002)
    R = len(srcs)
    t0 = time.perf_counter()
    for at in range(0, R, a.fill):
        eng.store_put(eng.query_sparse_topk(srcs[at:at + a.fill], a.topk, device=True)[0], append=at > 0)
    fill_s = time.perf_counter() - t0
    info = eng.store_info()
    steps = [rng.integers(0, R, size=a.batch) for _ in range(a.reps + 1)]

    # the caller's second copy of the CSR, which the torch baselines need: row_ptr, col, and for the mask the source of every edge
    t_rp = torch.from_numpy(np.ascontiguousarray(row_ptr, dtype=np.int64)).to(dev)
    t_col = torch.from_numpy(np.ascontiguousarray(col, dtype=np.int32)).to(dev).long()
    t_src = torch.repeat_interleave(torch.arange(n, device=dev), t_rp[1:] - t_rp[:-1])
    mask = torch.zeros(n, dtype=torch.bool, device=dev)
    inv = torch.empty(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def torch_mask(cols):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mask.zero_()
        mask[cols] = True
        inv[cols] = torch.arange(cols.numel(), device=dev)
        keep = mask[t_src] & mask[t_col]
        ei = torch.stack([inv[t_src[keep]], inv[t_col[keep]]])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ei

    def torch_rows(cols):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inv[cols] = torch.arange(cols.numel(), device=dev)
        first = t_rp[cols]
        deg = t_rp[cols + 1] - first
        scan = torch.cumsum(deg, 0) - deg
        src = torch.repeat_interleave(torch.arange(cols.numel(), device=dev), deg)
        eid = torch.arange(src.numel(), device=dev) + (first - scan)[src]
        dst = t_col[eid]
        keep = torch.isin(dst, cols)
        ei = torch.stack([src[keep], inv[dst[keep]]])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ei

    from fora_amd import capi
    ncs, scanned, edges = [], [], []
    call_ms = {s: [] for s in a.spans}
    bind_ms = {s: [] for s in a.spans}
    kern_ms = {s: [] for s in a.spans}
    mask_ms, rows_ms = [], []
    for i, rows in enumerate(steps):
        for s in a.spans:
            eng.set_option("sub_span", s)
            rp, cols, _ = eng.store_take_compact(rows, device=True)   # fora_hip_sparse_subgraph alone: the C call, nothing fetched
            e_c, s_c, ms_c = ctypes.c_int64(0), ctypes.c_uint64(0), ctypes.c_double(0)
            args = (eng._ctx, rp.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(rp.size - 1), ctypes.byref(e_c), ctypes.byref(s_c), ctypes.byref(ms_c))
            t0 = time.perf_counter()
            rc = eng._lib.fora_hip_sparse_subgraph(*args)
            dt_c = (time.perf_counter() - t0) * 1e3
            eng._chk(rc)
            rp, cols, _ = eng.store_take_compact(rows, device=True)   # Engine.sparse_subgraph: the call, three device tensors, the fetch
            t0 = time.perf_counter()
            sub_ptr, sub_col, sub_eid, st = eng.sparse_subgraph(rp, want_eid=True, device=True)
            dt = (time.perf_counter() - t0) * 1e3
            assert st["edges"] == e_c.value == sub_col.numel() and st["scanned"] == s_c.value
            if i:                                                     # (the first step warms up)
                call_ms[s].append(dt_c)
                bind_ms[s].append(dt)
                kern_ms[s].append(st["sub_ms"])
        cols = cols.long()
        dt_m, ei_m = torch_mask(cols)
        dt_r, ei_r = torch_rows(cols)
        ei = capi.subgraph_edge_index(sub_ptr, sub_col)
        assert torch.equal(ei, ei_m) and torch.equal(ei, ei_r)        # the same edges in the same order, three ways
        if i:
            mask_ms.append(dt_m)
            rows_ms.append(dt_r)
            ncs.append(int(cols.numel())); scanned.append(int(st["scanned"])); edges.append(int(st["edges"]))
    eng.set_option("sub_span", default_span)
    print(json.dumps({"tool": "subgraph_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "reps": a.reps, "sub_span": default_span,
                      "sources": R, "topk": a.topk, "store_rows": info["rows"], "fill_s": round(fill_s, 3), "batch": a.batch,
                      "nc": _summary(ncs, 0), "scanned": _summary(scanned, 0), "edges": _summary(edges, 0),
                      "call_ms": {str(s): _summary(call_ms[s]) for s in a.spans},
                      "binding_ms": {str(s): _summary(bind_ms[s]) for s in a.spans},
                      "kernel_ms": {str(s): _summary(kern_ms[s], 4) for s in a.spans},
                      "torch_mask_ms": _summary(mask_ms), "torch_rows_ms": _summary(rows_ms)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
