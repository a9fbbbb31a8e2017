"""The SWEEP CUT contract of include/fora_hip.h in plain Python ints, with nothing from the library: a sort, a dict of ranks,
a difference array and an exact fraction compare.  sweep_brute recomputes every prefix from set membership instead."""
import math
import struct

import numpy as np

FIX_ONE = 1 << 62


def thr_fix_of(t):
    return 1 if t <= 0 else max(1, math.ceil(math.ldexp(t, 62)))


def _order(row, deg, thr):
    support = [int(v) for v in np.flatnonzero(np.asarray(row) >= np.uint64(thr))]
    key = {v: int(row[v]) // max(int(deg[v]), 1) for v in support}
    return sorted(support, key=lambda v: (-key[v], v)), key


def _best(cut, vol, nnz):
    """(best, cut, vol, den, conductance): the prefix of least cut / den over den > 0, exact, ties to the smaller prefix"""
    b = None
    for j in range(len(cut)):
        den = min(vol[j], nnz - vol[j])
        if den > 0 and (b is None or cut[j] * b[3] < b[1] * den):
            b = (j + 1, cut[j], vol[j], den)
    if b is None:
        return 0, 0, 0, 0, 1.0
    return b + (float(b[1]) / float(b[3]),)


def sweep_row(row, row_ptr, col, thr, max_size=0):
    """row: the n fixed-point words of one ppr row.  Returns a dict: len, order, cut, vol (lists of L ints), best, cut_best,
    vol_best, den, conductance."""
    deg = np.diff(row_ptr)
    nnz = int(row_ptr[-1])
    order, _ = _order(row, deg, thr)
    n_sup = len(order)
    L = n_sup if max_size <= 0 else min(n_sup, int(max_size))
    order = order[:L]
    rank = {v: i for i, v in enumerate(order)}
    diff = [0] * L
    for i, u in enumerate(order):
        for v in col[int(row_ptr[u]):int(row_ptr[u + 1])]:
            r = rank.get(int(v), -1)
            if r < 0 or r > i:
                diff[i] += 1
                if r > i:
                    diff[r] -= 1
    cut, vol, c, s = [], [], 0, 0
    for i, u in enumerate(order):
        c += diff[i]
        s += int(deg[u])
        cut.append(c)
        vol.append(s)
    best, cb, vb, den, cond = _best(cut, vol, nnz)
    return {"len": n_sup, "order": order, "cut": cut, "vol": vol, "best": best, "cut_best": cb, "vol_best": vb, "den": den,
            "conductance": cond}


def dangling_row(s):
    """the row of a dangling source: the single entry (s, 2^62), no prefix with a denominator"""
    return {"len": 1, "order": [int(s)], "cut": [0], "vol": [0], "best": 0, "cut_best": 0, "vol_best": 0, "den": 0, "conductance": 1.0}


def sweep_brute(row, row_ptr, col, thr, max_size=0):
    """the same profile with cut and vol of every prefix recomputed from set membership"""
    deg = np.diff(row_ptr)
    nnz = int(row_ptr[-1])
    order, _ = _order(row, deg, thr)
    n_sup = len(order)
    L = n_sup if max_size <= 0 else min(n_sup, int(max_size))
    order = order[:L]
    cut, vol = [], []
    for j in range(L):
        S = set(order[:j + 1])
        cut.append(sum(1 for u in S for v in col[int(row_ptr[u]):int(row_ptr[u + 1])] if int(v) not in S))
        vol.append(sum(int(deg[u]) for u in S))
    best, cb, vb, den, cond = _best(cut, vol, nnz)
    return {"len": n_sup, "order": order, "cut": cut, "vol": vol, "best": best, "cut_best": cb, "vol_best": vb, "den": den,
            "conductance": cond}


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def planted_graph(seed=20261019, small=300, big=1699, nbrs=4, cross=60):
    """A symmetric two-block graph: every node draws `nbrs` random partners inside its block (about 2 * nbrs neighbours per
    node once the edges are mirrored), `cross` edges join the blocks, ids are permuted.  Returns (n, row_ptr, col, members of
    the small block)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = small + big
    pairs = set()
    for lo, size in ((0, small), (small, big)):
        for u in range(lo, lo + size):
            for v in lo + rng.choice(size, size=nbrs, replace=False):
                if int(v) != u:
                    pairs.add((min(u, int(v)), max(u, int(v))))
    while cross > 0:
        u, v = int(rng.integers(0, small)), int(small + rng.integers(0, big))
        if (u, v) not in pairs:
            pairs.add((u, v))
            cross -= 1
    perm = rng.permutation(n)
    e = np.array(sorted(pairs), dtype=np.int64)
    src = np.concatenate([perm[e[:, 0]], perm[e[:, 1]]])
    dst = np.concatenate([perm[e[:, 1]], perm[e[:, 0]]])
    o = np.lexsort((dst, src))
    src, dst = src[o], dst[o]
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=row_ptr[1:])
    return n, row_ptr, dst.astype(np.int32), np.sort(perm[:small]).astype(np.int32)
