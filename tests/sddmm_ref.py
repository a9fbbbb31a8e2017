"""The numpy twin of the SCORES (SDDMM) contract (include/fora_hip.h, fora_hip_sparse_sddmm): for every held entry e of row i
with id v, score_e = <A[i], B[v]> in the contract's order of additions -- 64 running sums q_l over the columns c == l (mod 64)
in ascending c from +0.0, then the tree q_l = q_l + q_{l+o} for o = 32 .. 1.  The loops run over column blocks and tree steps
and are vectorised over entries only; nothing here calls np.sum, np.dot or @ on floating point values.  numpy's elementwise
float64 multiply and add are single IEEE operations."""
import numpy as np

import propagate_ref as pr

LANES = 64


def widen(X, bf16=False):
    """an operand as float64: float32 widened, or uint16 bf16 bit patterns with bf16=True -- both exact"""
    return (pr.widen_bf16(X) if bf16 else np.asarray(X, dtype=np.float32)).astype(np.float64)


def entry_rows(row_ptr):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))


def tree_sum(terms, lanes=LANES):
    """[entries, d] float64 products -> [entries] scores by a group of `lanes` lanes (a power of two, lanes >= d unless it is
    64): q_l over c == l (mod 64) -- with lanes < 64 every lane has at most its one column -- then only the group's own steps
    of the tree, o = lanes / 2 .. 1"""
    e, d = terms.shape
    assert lanes == LANES or d <= lanes
    q = np.zeros((e, lanes), dtype=np.float64)
    for c0 in range(0, d, LANES):
        w = min(LANES, d - c0)
        q[:, :w] = q[:, :w] + terms[:, c0:c0 + w]
    o = lanes // 2
    while o:
        q[:, :o] = q[:, :o] + q[:, o:2 * o]
        o //= 2
    return q[:, 0].copy()


def sddmm_ref(row_ptr, ids, A, B, a_bf16=False, b_bf16=False, lanes=LANES):
    """(out64 [entries], out32 [entries]) of the pattern (row_ptr, ids) of a fetched sparse result, A ([nq, d]) and B
    ([n, d]), each float32 or uint16 bf16 bit patterns"""
    A64, B64 = widen(A, a_bf16), widen(B, b_bf16)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = A64[entry_rows(row_ptr)] * B64[np.asarray(ids, dtype=np.int64)]     # exact products
        out = tree_sum(terms, lanes)
        return out, out.astype(np.float32)


def sddmm_stats_ref(row_ptr, d, a_elt, b_elt):
    lens = np.diff(np.asarray(row_ptr, dtype=np.int64))
    return {"entries": int(lens.sum()), "segments": int(((lens + pr.SEG - 1) // pr.SEG).sum()), "max_row": int(lens.max()) if lens.size else 0,
            "bytes": int(lens.sum()) * d * (a_elt + b_elt)}


ROW_LENS = [5, 0, 1, 2, 255, 256, 257, 600, 3]      # the segment boundaries; row 1 is the empty one
EMPTY = 1


def injected_rows(n, seed=8600):
    """[nq, n] words: row i has ROW_LENS[i] entries at random nodes"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows_fix = np.zeros((len(ROW_LENS), n), dtype=np.uint64)
    for i, L in enumerate(ROW_LENS):
        at = rng.choice(n, size=L, replace=False)
        rows_fix[i, at] = rng.integers(1, (1 << 62) // 1024 + 1, size=L, dtype=np.uint64)
    return rows_fix


def operand(rows, d, ld, bf16, seed, nan_row=None):
    """[rows, d] as a view of a [rows, ld] array whose padding holds NaN patterns that must never be read; the same values
    at every pitch.  nan_row: a row of NaN -- the row of `a` that belongs to the empty held row"""
    X = pr.scaled_features(np.random.Generator(np.random.PCG64(seed)), rows, d)
    if bf16:
        wide = np.full((rows, ld), 0x7FC1, dtype=np.uint16)
        wide[:, :d] = pr.to_bf16_bits(X)
        if nan_row is not None:
            wide[nan_row] = 0x7FC1
    else:
        wide = np.full((rows, ld), np.nan, dtype=np.float32)
        wide[:, :d] = X
        if nan_row is not None:
            wide[nan_row] = np.nan
    return wide[:, :d]
