"""The numpy twin of EDGE ATTENTION, BACKWARD (fora_hip_subgraph_attention_bwd; include/fora_hip_edge_attention_bwd.h): per head
nothing but the composition the contract words -- EDGE SCORES (tests/subgraph_sddmm_ref.py) in float64, EDGE SOFTMAX backward
(tests/subgraph_softmax_ref.py) of them, SUBGRAPH PRODUCTS (tests/subgraph_prop_ref.py) along and across the forward call's
grouping with the float64 ds and with y as values.  No arithmetic of its own."""
import numpy as np

import subgraph_prop_ref as sr
import subgraph_sddmm_ref as ss
import subgraph_softmax_ref as sm


def backward(sub_ptr, sub_col, Q, K, V, G, y, heads=1, scale=1.0, by="row", q_kind=None, k_kind=None, v_kind=None, g_kind=None):
    """(dq64, dq32, dk64, dk32, dv64, dv32): dq and dk [nc, heads * d], dv [nc, heads * dv]; y [heads, edges] float32 or float64"""
    Q, K, V, G = sr.widen32(Q, q_kind), sr.widen32(K, k_kind), sr.widen32(V, v_kind), sr.widen32(G, g_kind)
    d, dv = Q.shape[1] // heads, V.shape[1] // heads
    along, across = (sr.propagate, sr.propagate_t) if by == "row" else (sr.propagate_t, sr.propagate)
    dy = ss.scores(sub_ptr, sub_col, *((G, V) if by == "row" else (V, G)), heads=heads)[0]    # g is read at the group
    with np.errstate(invalid="ignore", over="ignore"):
        ds = sm.backward(sub_ptr, sub_col, y, dy, scale, by)[0]
        part = lambda X, w, h: np.ascontiguousarray(X[:, h * w:(h + 1) * w])
        dq, dk, dv_ = (np.concatenate([product(sub_ptr, sub_col, part(X, w, h), values=vals[h])[0] for h in range(heads)], axis=1)
                       for product, X, w, vals in ((along, K, d, ds), (across, Q, d, ds), (across, G, dv, np.asarray(y))))
    return dq, dq.astype(np.float32), dk, dk.astype(np.float32), dv_, dv_.astype(np.float32)
