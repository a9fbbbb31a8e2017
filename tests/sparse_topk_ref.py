"""The twin of the top-k sparse rows (the SPARSE RESULTS, TOP-K contract of include/fora_hip.h), in numpy on u64.

A dense row w (u64 [n], words at 2^-62) under thr_fix and k keeps the k entries of {v : w[v] >= thr_fix} that come first
in (word descending, id ascending), listed in ascending id order.  ~w reverses the u64 order, and the stable sort keeps
ascending ids among equal words."""
import numpy as np


def topk_row(w, thr, k):
    """ids (int64, ascending) of the entries row `w` holds under threshold word `thr` and k >= 1"""
    w = np.asarray(w, dtype=np.uint64)
    cand = np.flatnonzero(w >= np.uint64(thr))
    if len(cand) > k:
        cand = np.sort(cand[np.argsort(~w[cand], kind="stable")[:k]])
    return cand


def topk_csr(rows, thr, k):
    """(row_ptr int64, ids int32, fix u64, lens of the supports) of the dense rows [nq, n]"""
    rows = np.asarray(rows, dtype=np.uint64)
    ids, fix, ptr, lens = [], [], [0], []
    for w in rows:
        keep = topk_row(w, thr, k)
        lens.append(int((w >= np.uint64(thr)).sum()))
        ids.append(keep.astype(np.int32))
        fix.append(w[keep])
        ptr.append(ptr[-1] + len(keep))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    return np.array(ptr, dtype=np.int64), cat(ids, np.int32), cat(fix, np.uint64), np.array(lens, dtype=np.int64)


def check_topk(rows, thr, k, row_ptr, ids, fix, sp=None, tk=None, live=None):
    """a fetched top-k result against the twin over the dense rows; the stats when given (live: mask of the rows that took a
    slot -- the top-k stats count those only, a dangling source's row is written without a selection)"""
    want_ptr, want_ids, want_fix, lens = topk_csr(rows, thr, k)
    assert (np.asarray(row_ptr) == want_ptr).all(), (list(row_ptr), list(want_ptr))
    assert (np.asarray(ids) == want_ids).all()
    assert (np.asarray(fix).view(np.uint64) == want_fix).all()
    if sp is not None:
        assert sp["entries"] == int(want_ptr[-1]) and sp["thr_fix"] == thr
        assert sp["max_row"] == (int(np.diff(want_ptr).max()) if len(lens) else 0)
    if tk is not None:
        lens_all, lens = lens, (lens if live is None else lens[np.asarray(live, dtype=bool)])
        assert tk["k"] == k and tk["support"] == int(lens.sum()) and tk["max_support"] == (int(lens.max()) if len(lens) else 0)
        assert tk["cut_rows"] == int((lens > k).sum()) == tk["lds_rows"] + tk["global_rows"]
        lens = lens_all
    return lens
