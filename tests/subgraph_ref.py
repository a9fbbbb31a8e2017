"""The numpy twin of SUBGRAPH (fora_hip_sparse_subgraph, include/fora_hip_ext.h): the subgraph the graph (row_ptr, col) induces
on cols, an ascending array of distinct node ids.  Per row of cols: the row's targets filtered by membership, ranked by
np.searchsorted, the edge ids by position."""
import numpy as np


def induced(row_ptr, col, cols):
    """(sub_ptr int64 [nc + 1], sub_col int32, sub_eid int64, scanned): row j = the out-edges of cols[j] with a target in cols,
    in the graph's order; scanned = the out-degrees of cols, added up"""
    row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    cols = np.asarray(cols, dtype=np.int32).reshape(-1)
    sub_ptr, sub_col, sub_eid, scanned = [0], [], [], 0
    for u in cols:
        eid = np.arange(row_ptr[u], row_ptr[u + 1], dtype=np.int64)
        keep = np.isin(col[eid], cols)
        sub_col.append(np.searchsorted(cols, col[eid][keep]).astype(np.int32))
        sub_eid.append(eid[keep])
        sub_ptr.append(sub_ptr[-1] + int(keep.sum()))
        scanned += eid.size
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    return np.array(sub_ptr, dtype=np.int64), cat(sub_col, np.int32), cat(sub_eid, np.int64), scanned
