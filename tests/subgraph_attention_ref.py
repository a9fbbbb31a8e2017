"""The numpy twin of EDGE ATTENTION (fora_hip_subgraph_attention; include/fora_hip_edge_attention.h): per head nothing but the
composition of the three existing twins -- EDGE SCORES (tests/subgraph_sddmm_ref.py) in float64, EDGE SOFTMAX
(tests/subgraph_softmax_ref.py) of them, SUBGRAPH PRODUCTS (tests/subgraph_prop_ref.py) with the float64 probabilities as values --
plus the two rules of the contract: a NaN (group, head) is written as the quiet NaN to its dv outputs, an empty group is +0.0."""
import numpy as np

import subgraph_prop_ref as sr
import subgraph_sddmm_ref as ss
import subgraph_softmax_ref as sm


def groups(sub_ptr, sub_col, by):
    """the group of every edge in the order of sub_col: its row, or by column its target"""
    sub_ptr = np.asarray(sub_ptr, dtype=np.int64)
    return np.repeat(np.arange(sub_ptr.size - 1), np.diff(sub_ptr)) if by == "row" else np.asarray(sub_col, dtype=np.int64)


def attention(sub_ptr, sub_col, Q, K, V, heads=1, scale=1.0, by="row", q_kind=None, k_kind=None, v_kind=None):
    """(out64, out32, y64, y32, nan_pairs): out [nc, heads * dv], y [heads, edges] in the order of sub_col"""
    Q, K, V = sr.widen32(Q, q_kind), sr.widen32(K, k_kind), sr.widen32(V, v_kind)
    dv = V.shape[1] // heads
    a, b = (Q, K) if by == "row" else (K, Q)                       # by column a is read at the edge's row: k
    y64, y32, nan_pairs = sm.forward(sub_ptr, sub_col, ss.scores(sub_ptr, sub_col, a, b, heads=heads)[0], scale, by)
    product, group = (sr.propagate if by == "row" else sr.propagate_t), groups(sub_ptr, sub_col, by)
    out64 = np.zeros((V.shape[0], heads * dv), dtype=np.float64)   # (an empty group: +0.0)
    with np.errstate(invalid="ignore"):
        for h in range(heads):
            cs = slice(h * dv, (h + 1) * dv)
            out64[:, cs] = product(sub_ptr, sub_col, np.ascontiguousarray(V[:, cs]), values=y64[h])[0]
            out64[np.unique(group[np.isnan(y64[h])]), cs] = np.nan  # a NaN (group, head): written, not computed
    return out64, out64.astype(np.float32), y64, y32, nan_pairs
