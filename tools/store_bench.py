#!/usr/bin/env python3
"""What a mini-batch of PPR rows costs from the row store against running the query again.  Two parts, one
JSON line.

  top-k store      the top --topk rows of --sources sources are put into the store in calls of --fill sources; then, per step of
                   --batch random rows, the legs
                     (a) store_take                              the rows become the held result: one copy on the GPU
                     (b) query_sparse_topk of the same sources   what a training loop pays without the store
                     (c) a plain-torch gather of the same rows   from the store's CSR fetched into device tensors
                   run alternately --reps times after one warm-up each; the line carries each leg's median and spread (min, max)
                   in ms per step -- a host clock around calls that end in a synchronise -- and take_kernel_ms, the library's
                   device events around k_store_take.  first_bwd_ms is sparse_attention_bwd on rows that have just been taken
                   (the transposition and the column plan are rebuilt inside the call), next_bwd_ms the call after it.
  thresholded      --thr-rows thresholded rows (threshold 1 / n) are stored and --thr-take random ones taken: take_kernel_ms and
                   the rate entries * 12 bytes / take_kernel_ms, beside a hipMemcpyAsync device-to-device copy of the same
                   byte count timed by events in the same run, and their ratio.
  spans            take_kernel_ms of both takes under every --spans value of the option "take_span" (median of --reps).

  python tools/store_bench.py --graph webstanford
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


def _memcpy_d2d_ms(nbytes, reps):
    """hipMemcpyAsync device-to-device of nbytes on torch's default (the null) stream, between events; ms per copy, per rep"""
    with open("/proc/self/maps") as f:               # the HIP runtime torch loaded, not a second one
        path = next(line.split()[-1] for line in f if "libamdhip64.so" in line)
    hip = ctypes.CDLL(path)
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    out = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = hip.hipMemcpyAsync(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), ctypes.c_size_t(nbytes), ctypes.c_int(3), None)
        b.record()
        torch.cuda.synchronize()
        if rc:
            raise RuntimeError(f"hipMemcpyAsync: {rc}")
        if i:                                          # (the first one warms up)
            out.append(a.elapsed_time(b))
    return out


def _torch_gather(rp, ids, fix, rows):
    """the rows `rows` of the device CSR (rp, ids, fix) as (row_ptr, ids, fix): what a user writes without the store"""
    lens = rp[rows + 1] - rp[rows]
    out_ptr = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=rp.device)
    torch.cumsum(lens, 0, out=out_ptr[1:])
    total = int(out_ptr[-1])
    idx = torch.repeat_interleave(rp[rows] - out_ptr[:-1], lens, output_size=total) + torch.arange(total, device=rp.device)
    return out_ptr, ids[idx], fix[idx]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--sources", type=int, default=20000)
    ap.add_argument("--fill", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=64)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--thr-rows", type=int, default=1000)
    ap.add_argument("--thr-take", type=int, default=250)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spans", type=int, nargs="+", default=[256, 1024, 2048, 4096, 16384])
    ap.add_argument("--d", type=int, default=64)
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
    default_span = eng.get_option("take_span")
    rng = np.random.Generator(np.random.PCG64(20261101))
    srcs = synth.query_set(n, a.sources, 20261002)
    R = len(srcs)

    def span_sweep(rows):
        out = {}
        for span in a.spans:
            eng.set_option("take_span", span)
            eng.store_take(rows)
            out[str(span)] = round(statistics.median([eng.store_take(rows)[1]["store_ms"] for _ in range(a.reps)]), 4)
        eng.set_option("take_span", default_span)
        return out

    # ---- the top-k store
    t0 = time.perf_counter()
    for at in range(0, R, a.fill):
        eng.store_put(eng.query_sparse_topk(srcs[at:at + a.fill], a.topk, device=True)[0], append=at > 0)
    fill_s = time.perf_counter() - t0
    info = eng.store_info()
    # its CSR in device tensors, for the torch leg: fetched through a take of every row
    rp_all, _ = eng.store_take(np.arange(R))
    ids_d = torch.empty(info["entries"], dtype=torch.int32, device=dev)
    fix_d = torch.empty(info["entries"], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    eng._chk(eng._lib.fora_hip_sparse_fetch(eng._ctx, ctypes.c_void_p(ids_d.data_ptr()), None, ctypes.c_void_p(fix_d.data_ptr()), ctypes.c_uint64(info["entries"])))
    rp_d = torch.from_numpy(rp_all).to(dev)
    steps = [rng.integers(0, R, size=a.batch) for _ in range(a.reps + 1)]
    kernel_ms, state = [], {}

    def leg_take(rows):
        state["rp"], st = eng.store_take(rows)
        kernel_ms.append(st["store_ms"])

    def leg_query(rows):
        eng.query_sparse_topk(srcs[rows], a.topk, device=True)
        torch.cuda.synchronize()

    def leg_torch(rows):
        state["gather"] = _torch_gather(rp_d, ids_d, fix_d, torch.from_numpy(rows).to(dev))
        torch.cuda.synchronize()

    legs = [("store_take", leg_take), ("query_sparse_topk", leg_query), ("torch_gather", leg_torch)]
    for _, f in legs:
        f(steps[0])
    kernel_ms.clear()
    ms = {name: [] for name, _ in legs}
    for rows in steps[1:]:
        for name, f in legs:
            t0 = time.perf_counter()
            f(rows)
            ms[name].append((time.perf_counter() - t0) * 1e3)
    # the three agree on the last step's rows
    leg_take(steps[-1])
    e = int(state["rp"][-1])
    got_ids, got_fix = np.zeros(e, np.int32), np.zeros(e, np.uint64)
    eng.sparse_fetch(got_ids, None, got_fix, cap=e)
    g_rp, g_ids, g_fix = (x.cpu().numpy() for x in state["gather"])
    assert (g_rp == state["rp"]).all() and (g_ids == got_ids).all() and (g_fix.view(np.uint64) == got_fix).all()
    # the first backward call after a take, and the one after it
    d = a.d
    Q = torch.randn(a.batch, d, device=dev)
    K = torch.randn(n, d, device=dev)
    V = torch.randn(n, d, device=dev)
    G = torch.randn(a.batch, d, device=dev)
    first_bwd, next_bwd, transpose_ms = [], [], []
    for rows in steps[1:]:
        rp = eng.store_take(rows)[0]
        y32 = eng.sparse_attention(rp, Q, K, V, want_y32=True)[2]
        for into in (first_bwd, next_bwd):
            t0 = time.perf_counter()
            st = eng.sparse_attention_bwd(rp, Q, K, V, G, y32)[6]
            into.append((time.perf_counter() - t0) * 1e3)
            if into is first_bwd:
                assert st["built"] == 1
                transpose_ms.append(st["transpose_ms"])
    topk = {"sources": R, "topk": a.topk, "store_rows": info["rows"], "store_entries": info["entries"], "fill_s": round(fill_s, 3), "batch": a.batch,
            "batch_entries": e, "ms": {k: _summary(v) for k, v in ms.items()}, "take_kernel_ms": _summary(kernel_ms[:a.reps], 4),
            "first_bwd_ms": _summary(first_bwd), "first_bwd_transpose_ms": _summary(transpose_ms, 4), "next_bwd_ms": _summary(next_bwd),
            "span_kernel_ms": span_sweep(steps[-1])}

    # ---- the thresholded store
    eng.store_clear()
    eng.sparse_clear()
    thr_srcs = srcs[:a.thr_rows]
    eng.store_put(eng.query_sparse(thr_srcs, device=True)[0])
    eng.sparse_clear()
    tinfo = eng.store_info()
    rows = rng.choice(len(thr_srcs), size=min(a.thr_take, len(thr_srcs)), replace=False)
    eng.store_take(rows)
    stats = [eng.store_take(rows)[1] for _ in range(a.reps)]
    tk_ms = [s["store_ms"] for s in stats]
    nbytes = int(stats[0]["entries"]) * 12
    cp_ms = _memcpy_d2d_ms(nbytes, a.reps)
    rate = lambda ms_: nbytes / (ms_ * 1e-3) / 1e12
    thr = {"store_rows": tinfo["rows"], "store_entries": tinfo["entries"], "max_row": tinfo["max_row"], "take_rows": int(len(rows)),
           "take_entries": int(stats[0]["entries"]), "bytes": nbytes, "take_kernel_ms": _summary(tk_ms, 4), "memcpy_d2d_ms": _summary(cp_ms, 4),
           "take_TBps": round(rate(statistics.median(tk_ms)), 3), "memcpy_TBps": round(rate(statistics.median(cp_ms)), 3),
           "take_over_memcpy": round(statistics.median(cp_ms) / statistics.median(tk_ms), 3), "span_kernel_ms": span_sweep(rows)}
    print(json.dumps({"tool": "store_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "reps": a.reps, "take_span": default_span,
                      "topk_store": topk, "thresholded_store": thr}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
