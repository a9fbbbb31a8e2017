"""The numpy twin of EDGE GAT and EDGE GAT, BACKWARD (fora_hip_subgraph_gat, fora_hip_subgraph_gat_bwd; include/fora_hip_edge_gat.h):
per head nothing but the composition the contract words -- one float64 addition, one multiplication and a select, then EDGE SOFTMAX
(tests/subgraph_softmax_ref.py), EDGE SCORES (tests/subgraph_sddmm_ref.py) and SUBGRAPH PRODUCTS (tests/subgraph_prop_ref.py)."""
import numpy as np

import subgraph_attention_ref as at
import subgraph_prop_ref as sr
import subgraph_sddmm_ref as ss
import subgraph_softmax_ref as sm


def pre_activation(sub_ptr, sub_col, el, er):
    """z [heads, edges]: el at the edge's row plus er at its column, in float64"""
    rows = at.groups(sub_ptr, sub_col, "row")
    with np.errstate(invalid="ignore"):
        return (el.astype(np.float64)[rows] + er.astype(np.float64)[np.asarray(sub_col, dtype=np.int64)]).T.copy()


def forward(sub_ptr, sub_col, el, er, V, heads=1, slope=0.2, by="row", el_kind=None, er_kind=None, v_kind=None):
    """(out64, out32, y64, y32, nan_pairs): out [nc, heads * dv], y [heads, edges] in the order of sub_col"""
    el, er, V = sr.widen32(el, el_kind), sr.widen32(er, er_kind), sr.widen32(V, v_kind)
    dv = V.shape[1] // heads
    z = pre_activation(sub_ptr, sub_col, el, er)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.where(z >= 0.0, z, z * slope)
    y64, y32, nan_pairs = sm.forward(sub_ptr, sub_col, s, 1.0, by)
    product, group = (sr.propagate if by == "row" else sr.propagate_t), at.groups(sub_ptr, sub_col, by)
    out64 = np.zeros((V.shape[0], heads * dv), dtype=np.float64)   # (an empty group: +0.0)
    with np.errstate(invalid="ignore"):
        for h in range(heads):
            cs = slice(h * dv, (h + 1) * dv)
            out64[:, cs] = product(sub_ptr, sub_col, np.ascontiguousarray(V[:, cs]), values=y64[h])[0]
            out64[np.unique(group[np.isnan(y64[h])]), cs] = np.nan  # a NaN (group, head): written, not computed
    return out64, out64.astype(np.float32), y64, y32, nan_pairs


def backward(sub_ptr, sub_col, el, er, V, G, y, heads=1, slope=0.2, by="row", el_kind=None, er_kind=None, v_kind=None, g_kind=None):
    """(del64, del32, der64, der32, dv64, dv32): d el and d er [nc, heads], dv [nc, heads * dv]; y [heads, edges] float32 or float64"""
    el, er, V, G = sr.widen32(el, el_kind), sr.widen32(er, er_kind), sr.widen32(V, v_kind), sr.widen32(G, g_kind)
    dv = V.shape[1] // heads
    along, across = (sr.propagate, sr.propagate_t) if by == "row" else (sr.propagate_t, sr.propagate)
    dy = ss.scores(sub_ptr, sub_col, *((G, V) if by == "row" else (V, G)), heads=heads)[0]    # g is read at the group
    z, ones = pre_activation(sub_ptr, sub_col, el, er), np.ones((V.shape[0], 1), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        ds = sm.backward(sub_ptr, sub_col, y, dy, 1.0, by)[0]
        dz = np.where(z >= 0.0, ds, ds * slope)
        d_group, d_other = (np.concatenate([product(sub_ptr, sub_col, ones, values=dz[h])[0] for h in range(heads)], axis=1) for product in (along, across))
        dv_ = np.concatenate([across(sub_ptr, sub_col, np.ascontiguousarray(G[:, h * dv:(h + 1) * dv]), values=np.asarray(y)[h])[0] for h in range(heads)], axis=1)
    dl, dr = (d_group, d_other) if by == "row" else (d_other, d_group)
    return dl, dl.astype(np.float32), dr, dr.astype(np.float32), dv_, dv_.astype(np.float32)
