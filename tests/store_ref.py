"""The numpy twin of the ROW STORE (include/fora_hip.h): take concatenates row slices of (row_ptr, ids, fix) in the caller's
order, load_ok says what fora_hip_store_load accepts, append puts rows behind rows.  Checker only."""
import numpy as np


def take(row_ptr, ids, fix, rows):
    """(row_ptr, ids, fix, vals) of the held result after fora_hip_store_take(rows) on a store (row_ptr, ids, fix)"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    R = row_ptr.size - 1
    if rows.size and (rows.min() < 0 or rows.max() >= R):
        raise IndexError("a take index outside the store")
    lens = row_ptr[rows + 1] - row_ptr[rows] if rows.size else np.zeros(0, dtype=np.int64)
    out_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    where = np.concatenate([np.arange(row_ptr[r], row_ptr[r + 1], dtype=np.int64) for r in rows] + [np.zeros(0, dtype=np.int64)])
    out_ids = np.asarray(ids, dtype=np.int32)[where]
    out_fix = np.asarray(fix, dtype=np.uint64)[where]
    return out_ptr, out_ids, out_fix, fix_to_vals(out_fix)


def fix_to_vals(fix):
    """vals[e] == ldexp((double)fix[e], -62): the u64 -> f64 conversion rounds to nearest even, the scaling is exact"""
    return np.ldexp(np.asarray(fix, dtype=np.uint64).astype(np.float64), -62)


def row_ptr_ok(row_ptr):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    return row_ptr.size >= 1 and row_ptr[0] == 0 and bool((np.diff(row_ptr) >= 0).all())


def first_bad_entry(row_ptr, ids, n):
    """the smallest entry fora_hip_store_load refuses -- an id outside [0, n), or not above the id before it in the same
    row -- or None"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    e = int(row_ptr[-1])
    bad = (ids[:e] < 0) | (ids[:e] >= n)
    inner = np.ones(e, dtype=bool)
    inner[row_ptr[:-1][row_ptr[:-1] < e]] = False          # a row's first entry has no id before it
    if e > 1:
        bad[1:] |= inner[1:] & (ids[:e - 1] >= ids[1:e])
    hit = np.flatnonzero(bad)
    return int(hit[0]) if hit.size else None


def load_ok(row_ptr, ids, n):
    return row_ptr_ok(row_ptr) and first_bad_entry(row_ptr, ids, n) is None


def append(a, b):
    """the store (row_ptr, ids, fix) `a` with the rows of `b` behind it"""
    return (np.concatenate([a[0], np.asarray(b[0][1:], dtype=np.int64) + a[0][-1]]).astype(np.int64),
            np.concatenate([a[1], b[1]]).astype(np.int32), np.concatenate([a[2], b[2]]).astype(np.uint64))
