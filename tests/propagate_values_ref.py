"""The numpy twin of the PROPAGATE WITH VALUES contract (include/fora_hip.h, fora_hip_sparse_propagate_vals and
fora_hip_sparse_propagate_t_vals): the sums of tests/propagate_ref.py and tests/propagate_t_ref.py with w_e = (double)values[e]
in place of the held word.  Nothing here calls np.sum, np.dot or @ on floating point values."""
import numpy as np

import propagate_ref as pr
import propagate_t_ref as pt


def _dense64(X, bf16):
    return (pr.widen_bf16(X) if bf16 else np.asarray(X, dtype=np.float32)).astype(np.float64)


def _values64(values):
    v = np.asarray(values)
    assert v.dtype in (np.float32, np.float64)
    return v.astype(np.float64)                       # f32 -> f64 is exact


def propagate_vals_ref(row_ptr, ids, values, H, bf16=False, seg=pr.SEG):
    """(out64 [nq, d], out32 [nq, d]): out[i] = sum over the entries e of row i of values[e] * H[ids[e]]"""
    H64, w = _dense64(H, bf16), _values64(values)
    ids = np.asarray(ids, dtype=np.int64)
    nq = len(row_ptr) - 1
    out = np.zeros((nq, H64.shape[1]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(nq):
            lo, hi = int(row_ptr[i]), int(row_ptr[i + 1])
            out[i] = pr.sum_row(w[lo:hi, None] * H64[ids[lo:hi]], seg)
        return out, out.astype(np.float32)


def transpose_order(ids):
    """pos: the held place of every entry of the transposition -- the stable sort by id that tests/propagate_t_ref.py makes"""
    return np.argsort(np.asarray(ids, dtype=np.int64), kind="stable")


def propagate_t_vals_ref(row_ptr, ids, values, G, n, bf16=False, seg=pr.SEG):
    """(out64 [n, d], out32 [n, d]): out[v] = sum over the held entries e with id v, by ascending row, of values[e] * G[row_e]"""
    G64, w = _dense64(G, bf16), _values64(values)
    ids = np.asarray(ids, dtype=np.int64)
    pos = transpose_order(ids)
    rows = pt.entry_rows(row_ptr).astype(np.int64)[pos]
    col_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ids, minlength=n), out=col_ptr[1:])
    out = np.zeros((n, G64.shape[1]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in np.flatnonzero(np.diff(col_ptr)):
            lo, hi = int(col_ptr[v]), int(col_ptr[v + 1])
            out[v] = pr.sum_row(w[pos[lo:hi], None] * G64[rows[lo:hi]], seg)
        return out, out.astype(np.float32)


def distinct_values(rng, entries, dtype):
    """one value per entry, all different, scaled over 2^+-20 so that a sum depends on the order of its additions and a
    value read from the wrong place changes bits"""
    draw = lambda cnt: np.ldexp(rng.standard_normal(cnt), rng.integers(-20, 21, size=cnt)).astype(dtype)
    v = draw(entries)
    while True:
        _, first = np.unique(v, return_index=True)
        again = np.setdiff1d(np.arange(entries), first)
        if not again.size:
            return v
        v[again] = draw(again.size)
