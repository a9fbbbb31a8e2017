"""The numpy twin of EDGE GATV2 (include/fora_hip_edge_gatv2.h): per head the four lines of the contract, then EDGE SOFTMAX
(tests/subgraph_softmax_ref.py) and the SUBGRAPH PRODUCTS (tests/subgraph_prop_ref.py), as tests/subgraph_gat_ref.py chains them."""
import numpy as np

import sddmm_ref
import subgraph_attention_ref as at
import subgraph_prop_ref as sr
import subgraph_softmax_ref as sm


def scores(sub_ptr, sub_col, xl, xr, att, heads=1, slope=0.2):
    # s [heads, edges] float64: xl at the edge's row, xr at its column, whichever the grouping
    rows, cols, d = at.groups(sub_ptr, sub_col, "row"), np.asarray(sub_col, dtype=np.int64), xl.shape[1] // heads
    s = np.zeros((heads, cols.size), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            u = xl.astype(np.float64)[rows, h * d:(h + 1) * d] + xr.astype(np.float64)[cols, h * d:(h + 1) * d]
            t = np.where(u >= 0.0, u, u * slope)
            s[h] = sddmm_ref.tree_sum(att.astype(np.float64)[h] * t)
    return s


def forward(sub_ptr, sub_col, xl, xr, att, V, heads=1, slope=0.2, by="row"):
    """(out64, out32, y64, y32, nan_pairs): out [nc, heads * dv], y [heads, edges] in the order of sub_col; float32 operands"""
    dv = V.shape[1] // heads
    y64, y32, nan_pairs = sm.forward(sub_ptr, sub_col, scores(sub_ptr, sub_col, xl, xr, att, heads, slope), 1.0, by)
    product, group = (sr.propagate if by == "row" else sr.propagate_t), at.groups(sub_ptr, sub_col, by)
    out64 = np.zeros((V.shape[0], heads * dv), dtype=np.float64)   # (an empty group: +0.0)
    with np.errstate(invalid="ignore"):
        for h in range(heads):
            cs = slice(h * dv, (h + 1) * dv)
            out64[:, cs] = product(sub_ptr, sub_col, np.ascontiguousarray(V[:, cs]), values=y64[h])[0]
            out64[np.unique(group[np.isnan(y64[h])]), cs] = np.nan  # a NaN (group, head): written, not computed
    return out64, out64.astype(np.float32), y64, y32, nan_pairs
