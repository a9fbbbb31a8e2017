"""The numpy twin of the PROPAGATE, TRANSPOSED contract (include/fora_hip.h, fora_hip_sparse_propagate_t): the transposition
of a fetched sparse result -- a stable sort of its entries by node id, so that a column lists its entries by ascending row --
and out[v][c] = sum over column v's entries of w'_e * G[row_e][c], summed as tests/propagate_ref.py sums a row.  Nothing
here calls np.sum, np.dot or @ on floating point values."""
import numpy as np

import propagate_ref as pr

SHORT, LDS_MAX = 64, 4096     # PROPT_SHORT, PROPT_LDS_MAX of fora_amd/csrc/fora_propt_plan.h


def entry_rows(row_ptr):
    """the row index of every entry"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int32), np.diff(row_ptr))


def transpose_ref(row_ptr, ids, fix, n):
    """(col_ptr [n + 1], rows, fix_t): the entries stably sorted by id -- row-major input makes that the row order"""
    ids = np.asarray(ids, dtype=np.int64)
    order = np.argsort(ids, kind="stable")
    col_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ids, minlength=n), out=col_ptr[1:])
    return col_ptr, entry_rows(row_ptr)[order], np.asarray(fix, dtype=np.uint64)[order]


def row_sums(row_ptr, fix):
    """S_i: the wrapping u64 sum of every row's words"""
    fix = np.asarray(fix, dtype=np.uint64)
    return np.array([sum(int(x) for x in fix[int(row_ptr[i]):int(row_ptr[i + 1])]) & ((1 << 64) - 1) for i in range(len(row_ptr) - 1)],
                    dtype=np.uint64)


def weights_t(rows, fix_t, S=None):
    """w'_e: the word as a double, with S divided by the double of its row's word sum -- one IEEE division"""
    w = pr.weights(fix_t)
    if S is None:
        return w
    with np.errstate(divide="ignore", invalid="ignore"):
        return w / pr.weights(np.asarray(S, dtype=np.uint64)[np.asarray(rows, dtype=np.int64)])


def column_terms(rows, fix_t, G64, S=None):
    """[len, d] the terms w'_e * g of one column, each one IEEE multiply"""
    return weights_t(rows, fix_t, S)[:, None] * G64[np.asarray(rows, dtype=np.int64)]


def propagate_t_ref(row_ptr, ids, fix, G, n, normalize=False, bf16=False, seg=pr.SEG):
    """(out64 [n, d], out32 [n, d]) of the rows (row_ptr, ids, fix) of a fetched sparse result and the gradient G ([nq, d]
    float32, or uint16 bf16 bit patterns with bf16=True)"""
    G64 = (pr.widen_bf16(G) if bf16 else np.asarray(G, dtype=np.float32)).astype(np.float64)
    col_ptr, rows, fix_t = transpose_ref(row_ptr, ids, fix, n)
    S = row_sums(row_ptr, fix) if normalize else None
    out = np.zeros((n, G64.shape[1]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in np.flatnonzero(np.diff(col_ptr)):
            lo, hi = int(col_ptr[v]), int(col_ptr[v + 1])
            out[v] = pr.sum_row(column_terms(rows[lo:hi], fix_t[lo:hi], G64, S), seg)
        return out, out.astype(np.float32)


COL_LENS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 600]


def injected_columns(n=2000, nq=601, empty_row=300, seed=7100):
    """(rows_fix [nq, n] words, col_lens [n]): dense rows whose COLUMNS have chosen lengths -- three nodes take each length of
    COL_LENS, every other node 0 .. 2 entries; row `empty_row` stays empty; words in [1, 2^62 / 1024], so no row sum wraps"""
    rng = np.random.Generator(np.random.PCG64(seed))
    live = np.setdiff1d(np.arange(nq), [empty_row])
    col_lens = rng.integers(0, 3, size=n)
    chosen = rng.choice(n, size=3 * len(COL_LENS), replace=False)
    col_lens[chosen] = np.repeat(COL_LENS, 3)
    rows_fix = np.zeros((nq, n), dtype=np.uint64)
    for v in range(n):
        L = int(col_lens[v])
        at = rng.choice(live, size=L, replace=False)
        rows_fix[at, v] = rng.integers(1, (1 << 62) // 1024 + 1, size=L, dtype=np.uint64)
    return rows_fix, col_lens


def csr_of(rows_fix):
    """(row_ptr, ids, fix) of dense rows: what a held sparse result of them at threshold 0 fetches"""
    nz = rows_fix != 0
    row_ptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    i, v = np.nonzero(nz)
    return row_ptr, v.astype(np.int32), rows_fix[i, v]


def tier_counts(col_ptr, cap=LDS_MAX):
    """the columns each sort tier takes under the option "propt_lds_cap" = cap: a run of one key is sorted by none, one longer
    than the cap in device memory, one of at most 64 keys by a wave, the others in LDS"""
    lens = np.diff(np.asarray(col_ptr, dtype=np.int64))
    cap = min(max(int(cap), 0), LDS_MAX)
    glob = (lens >= 2) & (lens > cap)
    short = (lens >= 2) & ~glob & (lens <= SHORT)
    return {"short_cols": int(short.sum()), "lds_cols": int(((lens >= 2) & ~glob & ~short).sum()), "global_cols": int(glob.sum())}


def propt_stats_ref(col_ptr, d, elt):
    lens = np.diff(np.asarray(col_ptr, dtype=np.int64))
    return {"entries": int(lens.sum()), "columns": int((lens > 0).sum()), "segments": int(((lens + pr.SEG - 1) // pr.SEG).sum()),
            "max_col": int(lens.max()) if lens.size else 0, "feat_bytes": int(lens.sum()) * d * elt}
