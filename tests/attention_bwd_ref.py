"""The numpy twin of the ATTENTION, BACKWARD contract (include/fora_hip.h, fora_hip_sparse_attention_bwd): per head the
composition of the twins of its steps with float64 in between -- dy = sddmm_ref of the head's slices of g and v, ds =
softmax_bwd_ref of (y_j, dy), dq = propagate_vals_ref of the k slice with ds, dk = propagate_t_vals_ref of the q slice with ds,
dv = propagate_t_vals_ref of the g slice with y_j in the caller's type.  Nothing is computed here a second way."""
import numpy as np

import propagate_t_ref as pt
import propagate_values_ref as pv
import sddmm_ref as sr
import softmax_ref as sm


def attention_bwd_ref(row_ptr, ids, Q, K, V, G, y, n, d, dv, heads, scale, q_bf16=False, k_bf16=False, v_bf16=False, g_bf16=False):
    """(dq64 [nq, heads * d], dk64 [n, heads * d], dv64 [n, heads * dv]); the float32 outputs are .astype(np.float32) of them.
    Q [nq, heads * d], K [n, heads * d], V [n, heads * dv], G [nq, heads * dv]: float32 or uint16 bf16 bit patterns each;
    y [heads, entries]: float32 or float64, what the forward call wrote"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    nq, e = len(row_ptr) - 1, int(row_ptr[-1])
    y = np.asarray(y)
    assert y.dtype in (np.float32, np.float64) and y.shape == (heads, e)
    assert Q.shape == (nq, heads * d) and K.shape == (n, heads * d) and V.shape == (n, heads * dv) and G.shape == (nq, heads * dv)
    dq = np.zeros((nq, heads * d), dtype=np.float64)
    dk = np.zeros((n, heads * d), dtype=np.float64)
    dvv = np.zeros((n, heads * dv), dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(heads):
            qs, vs = slice(j * d, (j + 1) * d), slice(j * dv, (j + 1) * dv)
            dy, _ = sr.sddmm_ref(row_ptr, ids, G[:, vs], V[:, vs], g_bf16, v_bf16)
            ds, _ = sm.softmax_bwd_ref(row_ptr, y[j], dy, scale)
            dq[:, qs], _ = pv.propagate_vals_ref(row_ptr, ids, ds, K[:, qs], k_bf16)
            dk[:, qs], _ = pv.propagate_t_vals_ref(row_ptr, ids, ds, Q[:, qs], n, q_bf16)
            dvv[:, vs], _ = pv.propagate_t_vals_ref(row_ptr, ids, y[j], G[:, vs], n, g_bf16)
    return dq, dk, dvv


def attention_bwd_stats_ref(row_ptr, ids, n, short_cap=sm.SEG):
    """the integer fields of fora_attn_bwd_stats for a call that wants dk or dv"""
    lens = np.diff(np.asarray(row_ptr, dtype=np.int64))
    cols = np.bincount(np.asarray(ids, dtype=np.int64), minlength=n)
    short_cap = min(max(int(short_cap), 0), sm.SEG)
    return {"entries": int(lens.sum()), "segments": int(((lens + sm.SEG - 1) // sm.SEG).sum()), "max_row": int(lens.max()) if lens.size else 0,
            "short_rows": int(((lens > 0) & (lens <= short_cap)).sum()), "long_rows": int((lens > short_cap).sum()),
            "columns": int((cols > 0).sum()), "max_col": int(cols.max()) if cols.size else 0,
            "short_cols": int(((cols > 0) & (cols <= short_cap)).sum()), "long_cols": int((cols > short_cap).sum())}


def injected(n):
    """[nq, n] words: the rows of propagate_t_ref.injected_columns(n) (columns of every length up to 600) stacked on those of
    softmax_ref.injected_rows(n) (rows of every length up to 600) -- every boundary of the row side and of the column side in
    one held result.  For n = 2000 the counts below hold; the fixture of the GPU tests asserts them."""
    return np.concatenate([pt.injected_columns(n)[0], sm.injected_rows(n)], axis=0)


INJECTED_2000 = {"rows": 612, "entries": 12862, "empty_rows": 2, "rows_over_256": 2, "row_lens": [63, 64, 65, 255, 256, 257, 600],
                 "empty_cols": 261, "cols_of_1": 556, "cols_of_256": 2, "cols_of_257": 2, "cols_over_256": 16, "max_col": 601}


def check_injected(rows_fix):
    """the counts of INJECTED_2000 on injected(2000)"""
    nz = rows_fix != 0
    rl, cl = nz.sum(axis=1), nz.sum(axis=0)
    c = INJECTED_2000
    assert rows_fix.shape == (c["rows"], 2000) and int(nz.sum()) == c["entries"]
    assert int((rl == 0).sum()) == c["empty_rows"] and int((rl > 256).sum()) == c["rows_over_256"]
    for L in c["row_lens"]:
        assert (rl == L).any(), L
    assert int((cl == 0).sum()) == c["empty_cols"] and int((cl == 1).sum()) == c["cols_of_1"]
    assert int((cl == 256).sum()) == c["cols_of_256"] and int((cl == 257).sum()) == c["cols_of_257"]
    assert int((cl > 256).sum()) == c["cols_over_256"] and int(cl.max()) == c["max_col"]
