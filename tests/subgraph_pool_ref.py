"""The numpy twin of SUBGRAPH POOL (fora_hip_subgraph_pool, fora_hip_subgraph_pool_bwd; include/fora_hip_pool.h).  Forward: the
definition on float64 -- a loop over the groups and an explicit scan of each for its first winner (all d columns of an entry at a
step).  Backward: column by column through the twins of the products with values (tests/propagate_values_ref.py): the weights are
T[e] = G[j(e), c] where arg[j(e), c] == e and 0.0 elsewhere, the operand a column of ones -- T * 1.0 is exact, so the order of
the sum is that twin's."""
import numpy as np

import propagate_values_ref as pv
import subgraph_prop_ref as sr

QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def forward(sub_ptr, sub_col, X, op="max", by="row", kind=None):
    """(out64, out32, arg int32), each [nc, d]"""
    sub_ptr = np.asarray(sub_ptr, dtype=np.int64)
    X64 = sr.widen32(X, kind).astype(np.float64)
    nc, d = sub_ptr.size - 1, X64.shape[1]
    if by == "row":
        ptr, src, edge = sub_ptr, np.asarray(sub_col, dtype=np.int64), np.arange(len(sub_col), dtype=np.int64)
    else:
        ptr, src, edge = sr.transpose(sub_ptr, sub_col)
    out, arg = np.zeros((nc, d), dtype=np.float64), np.full((nc, d), -1, dtype=np.int32)
    for j in range(nc):
        lo, hi = int(ptr[j]), int(ptr[j + 1])
        if lo == hi:
            continue
        best, e = X64[src[lo]].copy(), np.full(d, edge[lo], dtype=np.int32)
        for p in range(lo + 1, hi):                                   # ascending e: a later entry wins only where it is strictly better
            t = X64[src[p]]
            bn, tn = np.isnan(best), np.isnan(t)
            with np.errstate(invalid="ignore"):
                better = (tn & ~bn) | (t > best if op == "max" else t < best)
            best, e = np.where(better, t, best), np.where(better, np.int32(edge[p]), e)
        out[j], arg[j] = np.where(np.isnan(best), QNAN, best), e
    return out, out.astype(np.float32), arg


def backward(sub_ptr, sub_col, G, arg, by="row", kind=None):
    """(out64, out32) [nc, d]: by names the FORWARD call's grouping; the sum runs over the opposite side"""
    sub_ptr = np.asarray(sub_ptr, dtype=np.int64)
    G64 = sr.widen32(G, kind).astype(np.float64)
    nc, d = sub_ptr.size - 1, G64.shape[1]
    e = np.arange(len(sub_col), dtype=np.int64)
    group = np.repeat(np.arange(nc), np.diff(sub_ptr)) if by == "row" else np.asarray(sub_col, dtype=np.int64)
    ones, out = np.ones((nc, 1), dtype=np.float32), np.zeros((nc, d), dtype=np.float64)
    for c in range(d):
        T = np.where(np.asarray(arg)[group, c] == e, G64[group, c], 0.0)
        col = pv.propagate_t_vals_ref(sub_ptr, sub_col, T, ones, nc) if by == "row" else pv.propagate_vals_ref(sub_ptr, sub_col, T, ones)
        out[:, c] = col[0][:, 0]
    return out, out.astype(np.float32)
