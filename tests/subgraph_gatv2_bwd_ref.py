"""The numpy twin of EDGE GATV2, BACKWARD (include/fora_hip_edge_gatv2_bwd.h): the contract line by line in float64 -- dy, ds and dv
as tests/subgraph_gat_ref.py chains them, then u, t, w, du and a per edge, the sums of du over each side's groups in the order of
the SUBGRAPH PRODUCT (propagate_ref.sum_row: segments of 256) and d att through P_g and the tiles of 256 groups."""
import numpy as np

import propagate_ref as pr
import subgraph_attention_ref as at
import subgraph_prop_ref as sr
import subgraph_sddmm_ref as ss
import subgraph_softmax_ref as sm

TILE = 256  # FORA_GATV2_DATT_TILE


def backward(sub_ptr, sub_col, xl, xr, att, V, G, y, heads=1, slope=0.2, by="row"):
    """(dxl64, dxl32, dxr64, dxr32, datt64, datt32, dv64, dv32); float32 operands, y [heads, edges] float32 or float64"""
    sub_ptr, cols = np.asarray(sub_ptr, dtype=np.int64), np.asarray(sub_col, dtype=np.int64)
    nc, d, dv = V.shape[0], xl.shape[1] // heads, V.shape[1] // heads
    rows, across = at.groups(sub_ptr, sub_col, "row"), (sr.propagate_t if by == "row" else sr.propagate)
    dy = ss.scores(sub_ptr, sub_col, *((G, V) if by == "row" else (V, G)), heads=heads)[0]    # g is read at the group
    in_ptr, _, in_pos = sr.transpose(sub_ptr, sub_col)
    sides = {"row": (sub_ptr, np.arange(cols.size)), "col": (in_ptr, in_pos)}                 # a side's groups and its entries in its order
    dx, P = {side: np.zeros((nc, heads * d)) for side in sides}, np.zeros((nc, heads * d))
    with np.errstate(invalid="ignore", over="ignore"):
        ds = sm.backward(sub_ptr, sub_col, y, dy, 1.0, by)[0]
        dv_ = np.concatenate([across(sub_ptr, sub_col, np.ascontiguousarray(G[:, h * dv:(h + 1) * dv]), values=np.asarray(y)[h])[0] for h in range(heads)], axis=1)
        for h in range(heads):
            hs, a = slice(h * d, (h + 1) * d), att.astype(np.float64)[h]
            u = xl.astype(np.float64)[rows, hs] + xr.astype(np.float64)[cols, hs]
            du, ae = ds[h][:, None] * np.where(u >= 0.0, a, a * slope), ds[h][:, None] * np.where(u >= 0.0, u, u * slope)
            for side, (ptr, order) in sides.items():
                for grp in np.flatnonzero(np.diff(ptr)):
                    e = order[ptr[grp]:ptr[grp + 1]]
                    dx[side][grp, hs] = pr.sum_row(du[e])
                    if side == by:
                        P[grp, hs] = pr.sum_row(ae[e])
        datt = np.zeros(heads * d)
        for b in range(0, nc, TILE):
            tile = np.zeros(heads * d)
            for grp in range(b, min(nc, b + TILE)):
                tile = tile + P[grp]
            datt = datt + tile
    outs = (dx["row"], dx["col"], datt.reshape(heads, d), dv_)                                # xl is read at the edge's row, xr at its column
    return tuple(o for x in outs for o in (x, x.astype(np.float32)))
