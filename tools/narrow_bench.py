#!/usr/bin/env python3
"""What a narrower dense operand buys on the held rows: the same values as float32, bfloat16, float16 and FP8
E4M3 -- drawn as E4M3 codes, so that every type holds them exactly and all four runs compute the same sums -- through

  propagate   sparse_propagate over the full thresholded rows of --queries sources (README's 17 M-entry case on webstanford),
              a device resident H [n, d]: the gather and combine kernels' device events;
  attention   sparse_attention over the rows cut to their --topk largest entries, K and V [n, heads * d] in the type, Q float32:
              the call's device events.

Every type is warmed up once; then the types run alternately --reps times, and a line carries each type's median and spread
(min, max) in ms, the bytes of the operand that the entries read (entries * d * element size), and that over the median gather
time.  The outputs of the four types are compared bit for bit before anything is timed.

  python tools/narrow_bench.py --graph webstanford
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # before the library is loaded: one HIP runtime in the process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TYPES = (("f32", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16), ("e4m3", torch.float8_e4m3fn))


def _summary(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def _e4m3_codes(rng, shape):
    """finite codes of moderate exponent, both signs"""
    return ((rng.integers(0, 2, size=shape) << 7) | (rng.integers(4, 10, size=shape) << 3) | rng.integers(0, 8, size=shape)).astype(np.uint8)


def _as_types(codes, dev):
    """{name: tensor}: the same values in every type (E4M3 -> any of the others is exact)"""
    t8 = torch.from_numpy(codes).to(dev).view(torch.float8_e4m3fn)
    wide = t8.to(torch.float32)
    return {name: (t8 if dt == torch.float8_e4m3fn else wide.to(dt)) for name, dt in TYPES}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--attn-d", type=int, default=64)
    ap.add_argument("--heads", type=int, default=8)
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
    srcs = synth.query_set(n, a.queries, 20261001)
    nq = len(srcs)
    rng = np.random.Generator(np.random.PCG64(20261021))
    base = {"tool": "narrow_bench", "graph": a.graph, "n": n, "m": m, "epsilon": a.epsilon, "queries": a.queries, "reps": a.reps}

    # ---- propagate over the thresholded rows
    rp = eng.query_sparse(srcs, device=True)[0].cpu().numpy()
    entries = int(rp[-1])
    H = _as_types(_e4m3_codes(rng, (n, a.d)), dev)
    out32 = {name: torch.empty((nq, a.d), dtype=torch.float32, device=dev) for name, _ in TYPES}
    stats = {}
    for name, _ in TYPES:                                    # warm-up, and the four outputs are one
        _, _, stats[name] = eng.sparse_propagate(rp, H[name], want64=False, out32=out32[name])
        assert torch.equal(out32[name].view(torch.int32), out32["f32"].view(torch.int32)), name
    ms = {name: {"gather": [], "combine": []} for name, _ in TYPES}
    for _ in range(a.reps):
        for name, _ in TYPES:
            _, _, st = eng.sparse_propagate(rp, H[name], want64=False, out32=out32[name])
            ms[name]["gather"].append(st["gather_ms"])
            ms[name]["combine"].append(st["combine_ms"])
    for name, _ in TYPES:
        g = _summary(ms[name]["gather"])
        print(json.dumps({**base, "case": "propagate", "rows": "thresholded", "type": name, "d": a.d, "entries": entries,
                          "feat_bytes": int(stats[name]["feat_bytes"]), "gather_ms": g, "combine_ms": _summary(ms[name]["combine"]),
                          "gather_GBps": round(stats[name]["feat_bytes"] / g["median"] / 1e6, 1)}), flush=True)

    # ---- attention over the top-k rows
    rp = eng.query_sparse_topk(srcs, a.topk, device=True)[0].cpu().numpy()
    entries = int(rp[-1])
    d, heads = a.attn_d, a.heads
    w = heads * d
    Q = torch.from_numpy(rng.standard_normal((nq, w), dtype=np.float32) * 0.25).to(dev)
    K, V = _as_types(_e4m3_codes(rng, (n, w)), dev), _as_types(_e4m3_codes(rng, (n, w)), dev)
    out32 = {name: torch.empty((nq, w), dtype=torch.float32, device=dev) for name, _ in TYPES}
    for name, _ in TYPES:
        eng.sparse_attention(rp, Q, K[name], V[name], heads=heads, want64=False, out32=out32[name])
        assert torch.equal(out32[name].view(torch.int32), out32["f32"].view(torch.int32)), name
    ms = {name: [] for name, _ in TYPES}
    for _ in range(a.reps):
        for name, _ in TYPES:
            st = eng.sparse_attention(rp, Q, K[name], V[name], heads=heads, want64=False, out32=out32[name])[4]
            ms[name].append(st["attn_ms"])
    for name, dt in TYPES:
        print(json.dumps({**base, "case": "attention", "rows": f"topk{a.topk}", "type": name, "d": d, "dv": d, "heads": heads, "entries": entries,
                          "kv_bytes": entries * 2 * w * dt.itemsize, "short_rows": int(st["short_rows"]), "long_rows": int(st["long_rows"]),
                          "attn_ms": _summary(ms[name])}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
