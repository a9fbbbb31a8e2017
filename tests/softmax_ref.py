"""The numpy twin of the ROW SOFTMAX contract (include/fora_hip.h, fora_hip_sparse_softmax / fora_hip_sparse_softmax_bwd): the
defined exponential exp_def, the row maximum, the row sum in the contract's order -- 64 running sums q_l over the
segment-relative positions j == l (mod 64) in ascending j from +0.0, the tree q_l = q_l + q_{l+o} for o = 32 .. 1, the
segments of 256 entries added one after the other -- and the division; and the gradient in the same order.  Elementwise
numpy operations only: nothing here calls np.sum, np.exp, np.dot or a reduction of floating point values (the maximum is a
fold of elementwise np.maximum: any order gives its bits).  numpy's elementwise float64 multiply, add, subtract, divide and
rint are single IEEE operations."""
import math

import numpy as np

LANES = 64
SEG = 256
LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42feep-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
COEF = [1.0 / float(math.factorial(j)) for j in range(14)]      # one IEEE division of two exact doubles each (13! < 2^53)
QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def exp_def(t):
    """exp_def of the contract, for t <= 0 or -inf (any shape); every bit defined"""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(all="ignore"):
        live = t >= -708.0                                       # false for -inf (and for a NaN, which never comes)
        tt = np.where(live, t, 0.0)
        k = np.rint(tt * LOG2E)
        r = (tt - k * LN2_HI) - k * LN2_LO
        p = np.full(t.shape, COEF[13], dtype=np.float64)
        for j in range(12, -1, -1):
            p = p * r + COEF[j]
        two_k = ((k.astype(np.int64) + 1023) << 52).view(np.float64)
        return np.where(live, p * two_k, 0.0)


def row_sum(terms):
    """the contract's sum of one row's terms (a one-dimensional float64 array, at least one element)"""
    S = None
    with np.errstate(all="ignore"):
        for s0 in range(0, terms.size, SEG):
            seg = terms[s0:s0 + SEG]
            q = np.zeros(LANES, dtype=np.float64)
            for j0 in range(0, seg.size, LANES):
                w = min(LANES, seg.size - j0)
                q[:w] = q[:w] + seg[j0:j0 + w]
            o = LANES // 2
            while o:
                q[:o] = q[:o] + q[o:2 * o]
                o //= 2
            S = q[0] if S is None else S + q[0]
    return S


def _row_max(x):
    while x.size > 1:
        h = x.size // 2
        x = np.concatenate([np.maximum(x[:h], x[h:2 * h]), x[2 * h:]])
    return x[0]


def softmax_ref(row_ptr, scores, scale=1.0):
    """(out64, out32, nan_rows) of the forward call: scores float32 or float64 [entries]"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    scores = np.asarray(scores)
    assert scores.dtype in (np.float32, np.float64)
    out = np.zeros(int(row_ptr[-1]), dtype=np.float64)
    nan_rows = 0
    with np.errstate(all="ignore"):
        x = scores.astype(np.float64) * np.float64(scale)
        for i in range(len(row_ptr) - 1):
            a, b = int(row_ptr[i]), int(row_ptr[i + 1])
            if a == b:
                continue
            xr = x[a:b]
            m = np.inf if np.isnan(xr).any() else _row_max(xr)      # (a NaN entry, +inf and all -inf: the three NaN rows)
            if np.isinf(m):
                out[a:b] = QNAN
                nan_rows += 1
                continue
            p = exp_def(xr - m)
            out[a:b] = p / row_sum(p)
        return out, out.astype(np.float32), nan_rows


def softmax_bwd_ref(row_ptr, y, grad, scale=1.0):
    """(out64, out32) of the backward call: y and grad float32 or float64 [entries], each its own type"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    y, grad = np.asarray(y), np.asarray(grad)
    assert y.dtype in (np.float32, np.float64) and grad.dtype in (np.float32, np.float64)
    out = np.zeros(int(row_ptr[-1]), dtype=np.float64)
    with np.errstate(all="ignore"):
        y64, g64 = y.astype(np.float64), grad.astype(np.float64)
        t = y64 * g64
        for i in range(len(row_ptr) - 1):
            a, b = int(row_ptr[i]), int(row_ptr[i + 1])
            if a == b:
                continue
            D = row_sum(t[a:b])
            out[a:b] = ((g64[a:b] - D) * y64[a:b]) * np.float64(scale)
        return out, out.astype(np.float32)


def softmax_stats_ref(row_ptr, short_cap=SEG):
    lens = np.diff(np.asarray(row_ptr, dtype=np.int64))
    short_cap = min(max(int(short_cap), 0), SEG)
    return {"entries": int(lens.sum()), "segments": int(((lens + SEG - 1) // SEG).sum()), "max_row": int(lens.max()) if lens.size else 0,
            "short_rows": int(((lens > 0) & (lens <= short_cap)).sum()), "long_rows": int((lens > short_cap).sum())}


ROW_LENS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 600, 3]      # the lane and segment boundaries; row 0 is the empty one
EMPTY = 0


def injected_rows(n, lens=ROW_LENS, seed=8700):
    """[nq, n] words: row i has lens[i] entries at random nodes"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows_fix = np.zeros((len(lens), n), dtype=np.uint64)
    for i, L in enumerate(lens):
        at = rng.choice(n, size=L, replace=False)
        rows_fix[i, at] = rng.integers(1, (1 << 62) // 1024 + 1, size=L, dtype=np.uint64)
    return rows_fix


def exp_grid(seed=8710, random_points=4000):
    """the points exp_def is pinned at: the ends of its range and their neighbours, the points whose t * LOG2E lies closest to
    a half-integer (where rint decides k), multiples of LN2_HI (r = a rounding error away from 0), -inf, and random points"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pts = [0.0, -0.0, -708.0, np.nextafter(-708.0, 0.0), np.nextafter(-708.0, -np.inf), -np.inf, -709.0, -1e300,
           -5e-324, -2.0 ** -1022, -1e-300, -2.0 ** -53, -2.0 ** -30]
    for h in list(range(1, 40)) + [101, 511, 1000, 1021, 2041, 2042, 2043]:      # k + 1/2 = h / 2 for odd h: t near -(h / 2) * ln 2
        if h % 2 == 0:
            continue
        t = -(h / 2.0) / LOG2E
        near = [t]
        for _ in range(3):
            near = [np.nextafter(near[0], 0.0)] + near + [np.nextafter(near[-1], -np.inf)]
        near.sort(key=lambda v: abs(abs(v * LOG2E) - h / 2.0))
        pts += near[:3]
    for k in (1, 2, 3, 7, 64, 100, 511, 1000, 1021):
        pts += [-k * LN2_HI, np.nextafter(-k * LN2_HI, 0.0), np.nextafter(-k * LN2_HI, -np.inf)]
    pts = [v for v in pts if v <= 0.0]
    rnd = np.concatenate([-rng.random(random_points // 4) * 708.0, -rng.random(random_points // 4) * 40.0, -rng.random(random_points // 4),
                          -np.exp2(-rng.random(random_points // 4) * 60.0)])
    return np.concatenate([np.array(pts, dtype=np.float64), rnd])
