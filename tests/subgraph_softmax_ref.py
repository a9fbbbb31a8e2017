"""The numpy twin of EDGE SOFTMAX (fora_hip_subgraph_softmax, fora_hip_subgraph_softmax_bwd; include/fora_hip_edge_softmax.h): per
head, the twin of ROW SOFTMAX (tests/softmax_ref.py) over the groups of the held subgraph's edges -- by row the CSR itself, by
column the transposition of tests/subgraph_prop_ref.py: the values gathered through in_pos, the result scattered back."""
import numpy as np

import softmax_ref
import subgraph_prop_ref as sr


def _per_head(sub_ptr, sub_col, by, fn, *operands):
    ptr, pos = np.asarray(sub_ptr, dtype=np.int64), None
    if by == "col":
        ptr, _, pos = sr.transpose(sub_ptr, sub_col)
    out, nan_groups = np.zeros(operands[0].shape, dtype=np.float64), 0
    for h in range(out.shape[0]):
        res = fn(ptr, *[x[h] if pos is None else x[h][pos] for x in operands])
        out[h][slice(None) if pos is None else pos] = res[0]
        nan_groups += res[2] if len(res) > 2 else 0
    return out, out.astype(np.float32), nan_groups


def forward(sub_ptr, sub_col, scores, scale=1.0, by="row"):
    """(out64, out32, nan_groups): scores float32 or float64 [heads, edges] in the order of sub_col"""
    return _per_head(sub_ptr, sub_col, by, lambda ptr, s: softmax_ref.softmax_ref(ptr, s, scale), np.asarray(scores))


def backward(sub_ptr, sub_col, y, g, scale=1.0, by="row"):
    """(out64, out32): y and g [heads, edges], float32 or float64 each"""
    return _per_head(sub_ptr, sub_col, by, lambda ptr, yy, gg: softmax_ref.softmax_bwd_ref(ptr, yy, gg, scale), np.asarray(y), np.asarray(g))[:2]
