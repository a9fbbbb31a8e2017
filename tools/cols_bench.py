#!/usr/bin/env python3
"""What a training step over a mini-batch of stored PPR rows costs over the batch's own columns against over all n nodes
(DESIGN.md 5.21).  One JSON line.

  The top --topk rows of --sources sources are put into the row store in calls of --fill sources.  A step is --batch random
  rows.  Every comparison is the uncompacted path in the same run; legs run alternately --reps times after one warm-up each,
  and the line carries each leg's median and spread (min, max) in ms -- a host clock around calls that end in a synchronise
  unless named a kernel time, which are the library's device events.

  nc                 the columns of the steps' batches
  compact            per call under every --blocks value of the option "cols_block": compact_call_ms, fora_hip_sparse_compact
                     alone (the C call through ctypes, nothing fetched); compact_ms, Engine.sparse_compact(device=True) (that
                     call, a device tensor made for cols, a device synchronise and the fetch); cols_kernel_ms, the call's cols_ms
  first_bwd          the first sparse_attention_bwd (d = --d per head, every --heads) after take + compact, with K[cols] and
                     V[cols], against after take alone with K and V over all n nodes
  step               take, compact, the gather X[cols] in torch, forward, backward (compacted) against take, forward, backward
                     over [n, d] (uncompacted); torch_ops.ppr_attention_fused(backward="fused")

  python tools/cols_bench.py --graph webstanford
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
    ap.add_argument("--blocks", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--heads", type=int, nargs="+", default=[1, 8])
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps: at least 3")

    import fora_amd
    from fora_amd import synth
    from fora_amd.torch_ops import ppr_attention_fused
    n, m, row_ptr, col = synth.preset(a.graph)
    eng = fora_amd.Engine(0)
    dev = torch.device("cuda", eng.device)
    eng.set_graph(n, m, row_ptr, col)
    eng.set_params(alpha=0.2, epsilon=a.epsilon, seed=0x464F5241)
    default_block = eng.get_option("cols_block")
    rng = np.random.Generator(np.random.PCG64(20261201))
    srcs = synth.query_set(n, a.sources, 20261002)
    R = len(srcs)
    t0 = time.perf_counter()
    for at in range(0, R, a.fill):
        eng.store_put(eng.query_sparse_topk(srcs[at:at + a.fill], a.topk, device=True)[0], append=at > 0)
    fill_s = time.perf_counter() - t0
    info = eng.store_info()
    steps = [rng.integers(0, R, size=a.batch) for _ in range(a.reps + 1)]

    # ---- the compaction alone, under every block size
    from fora_amd import capi
    ncs, entries = [], 0
    call_ms = {b: [] for b in a.blocks}
    compact_ms = {b: [] for b in a.blocks}
    cols_ms = {b: [] for b in a.blocks}
    for i, rows in enumerate(steps):
        for b in a.blocks:
            eng.set_option("cols_block", b)
            rp = eng.store_take(rows)[0]                   # fora_hip_sparse_compact alone: the C call, nothing fetched
            nc_c, st_c = ctypes.c_int64(0), capi.ColsStats()
            args = (eng._ctx, rp.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(rp.size - 1), ctypes.byref(nc_c), ctypes.byref(st_c))
            t0 = time.perf_counter()
            rc = eng._lib.fora_hip_sparse_compact(*args)
            dt_c = (time.perf_counter() - t0) * 1e3
            eng._chk(rc)
            rp = eng.store_take(rows)[0]                   # Engine.sparse_compact: the call, a device tensor made for cols, its fetch
            t0 = time.perf_counter()
            cols, st = eng.sparse_compact(rp, device=True)
            dt = (time.perf_counter() - t0) * 1e3
            assert st["cols"] == nc_c.value == cols.numel()
            if i:                                          # (the first step warms up)
                call_ms[b].append(dt_c)
                compact_ms[b].append(dt)
                cols_ms[b].append(st["cols_ms"])
        if i:
            ncs.append(int(st["cols"]))
            entries = int(st["entries"])
    eng.set_option("cols_block", default_block)

    d = a.d
    per_heads = {}
    for heads in a.heads:
        w = heads * d
        scale = float(d) ** -0.5
        Q = torch.randn(a.batch, w, device=dev)
        K = torch.randn(n, w, device=dev)
        V = torch.randn(n, w, device=dev)
        G = torch.randn(a.batch, w, device=dev)
        torch.cuda.synchronize()

        # ---- the first backward call on rows that have just become held
        def first_bwd(rows, compacted):
            rp = eng.store_take(rows)[0]
            if compacted:
                cols = eng.sparse_compact(rp, device=True)[0].long()
                Kx, Vx = K[cols], V[cols]
            else:
                Kx, Vx = K, V
            y32 = eng.sparse_attention(rp, Q, Kx, Vx, heads=heads, scale=scale, want_y32=True)[2]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = eng.sparse_attention_bwd(rp, Q, Kx, Vx, G, y32, heads=heads, scale=scale)[6]
            dt = (time.perf_counter() - t0) * 1e3
            assert st["built"] == 1 and st["plan_cached"] == 0
            return dt, st["transpose_ms"], st["attn_ms"]

        # ---- a whole step through autograd
        def step(rows, compacted):
            Kp, Vp = K.detach().requires_grad_(True), V.detach().requires_grad_(True)
            Qp = Q.detach().requires_grad_(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if compacted:
                rp, cols, _ = eng.store_take_compact(rows, device=True)
                cols = cols.long()
                Kx, Vx = Kp[cols], Vp[cols]
            else:
                rp = eng.store_take(rows)[0]
                Kx, Vx = Kp, Vp
            ppr_attention_fused(eng, rp, Qp, Kx, Vx, scale=scale, heads=heads, backward="fused").backward(G)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        fb = {True: [], False: []}
        fb_t = {True: [], False: []}
        fb_k = {True: [], False: []}
        stp = {True: [], False: []}
        for i, rows in enumerate(steps):
            for compacted in (True, False):
                dt, tr, at = first_bwd(rows, compacted)
                if i:
                    fb[compacted].append(dt); fb_t[compacted].append(tr); fb_k[compacted].append(at)
        for i, rows in enumerate(steps):
            for compacted in (True, False):
                dt = step(rows, compacted)
                if i:
                    stp[compacted].append(dt)
        per_heads[str(heads)] = {
            "first_bwd_ms": {"compacted": _summary(fb[True]), "uncompacted": _summary(fb[False])},
            "first_bwd_transpose_ms": {"compacted": _summary(fb_t[True], 4), "uncompacted": _summary(fb_t[False], 4)},
            "first_bwd_attn_ms": {"compacted": _summary(fb_k[True], 4), "uncompacted": _summary(fb_k[False], 4)},
            "step_ms": {"compacted": _summary(stp[True]), "uncompacted": _summary(stp[False])},
            "step_ratio": round(statistics.median(stp[False]) / statistics.median(stp[True]), 2),
        }
        del Q, K, V, G
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "cols_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "reps": a.reps, "cols_block": default_block,
                      "sources": R, "topk": a.topk, "store_rows": info["rows"], "store_entries": info["entries"], "fill_s": round(fill_s, 3),
                      "batch": a.batch, "batch_entries": entries, "nc": _summary(ncs, 0), "d": d,
                      "compact_call_ms": {str(b): _summary(call_ms[b]) for b in a.blocks},
                      "compact_ms": {str(b): _summary(compact_ms[b]) for b in a.blocks},
                      "cols_kernel_ms": {str(b): _summary(cols_ms[b], 4) for b in a.blocks}, "heads": per_heads}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
