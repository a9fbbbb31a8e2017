"""The numpy twin of the ATTENTION contract (include/fora_hip.h, fora_hip_sparse_attention): per head the composition of the
twins of its three steps with float64 in between -- sddmm_ref on the head's column slices of Q and K, softmax_ref on those
float64 scores, propagate_vals_ref of the head's slice of V with the float64 y as the values -- plus what the contract adds:
a NaN (row, head) is written as the quiet NaN in y and in its dv outputs, and y comes out head by head.  Nothing is computed
here a second way."""
import numpy as np

import propagate_values_ref as pv
import sddmm_ref as sr
import softmax_ref as sm

QNAN = sm.QNAN


def attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, scale, q_bf16=False, k_bf16=False, v_bf16=False):
    """(out64 [nq, heads * dv], out32, y64 [heads, entries], y32, nan_rows): Q [nq, heads * d], K [n, heads * d] and V
    [n, heads * dv], each float32 or uint16 bf16 bit patterns; nan_rows counts (row, head) pairs"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    nq, e = len(row_ptr) - 1, int(row_ptr[-1])
    assert Q.shape == (nq, heads * d) and K.shape[1] == heads * d and V.shape[1] == heads * dv
    out = np.zeros((nq, heads * dv), dtype=np.float64)
    y = np.zeros((heads, e), dtype=np.float64)
    nan_rows = 0
    for j in range(heads):
        s64, _ = sr.sddmm_ref(row_ptr, ids, Q[:, j * d:(j + 1) * d], K[:, j * d:(j + 1) * d], q_bf16, k_bf16)
        y[j], _, nr = sm.softmax_ref(row_ptr, s64, scale)
        o, _ = pv.propagate_vals_ref(row_ptr, ids, y[j], V[:, j * dv:(j + 1) * dv], v_bf16)
        for i in range(nq):                                  # the NaN rows are written, not computed
            a, b = int(row_ptr[i]), int(row_ptr[i + 1])
            if b > a and np.isnan(y[j, a]):
                assert np.isnan(y[j, a:b]).all()
                o[i] = QNAN
        nan_rows += nr
        out[:, j * dv:(j + 1) * dv] = o
    return out, out.astype(np.float32), y, y.astype(np.float32), nan_rows


def attention_stats_ref(row_ptr, short_cap=sm.SEG):
    lens = np.diff(np.asarray(row_ptr, dtype=np.int64))
    short_cap = min(max(int(short_cap), 0), sm.SEG)
    return {"entries": int(lens.sum()), "segments": int(((lens + sm.SEG - 1) // sm.SEG).sum()), "max_row": int(lens.max()) if lens.size else 0,
            "short_rows": int(((lens > 0) & (lens <= short_cap)).sum()), "long_rows": int((lens > short_cap).sum())}


def scores_operands(rng, nq, n, d, heads, spread=30.0):
    """Q [nq, heads * d] and K [n, heads * d] as float32 whose scores are spread over about +-spread (three standard deviations;
    exp spans 26 decades inside a row, so the order of the additions shows in the bits): entries of K of order 1, entries of
    Q of order spread / (3 sqrt(d)).  The products of two float32 are exact in float64 and fill 48 bits, so their sums round."""
    Q = (rng.standard_normal((nq, heads * d)) * (spread / 3.0 / np.sqrt(d))).astype(np.float32)
    K = rng.standard_normal((n, heads * d)).astype(np.float32)
    return Q, K


def padded(X, ld, bf16):
    """X as a view of a [rows, ld] array whose padding holds NaN patterns that must never be read (uint16 bf16 bit patterns with
    bf16: the values rounded to bf16 first)"""
    import propagate_ref as pr
    rows, w = X.shape
    if bf16:
        wide = np.full((rows, ld), 0x7FC1, dtype=np.uint16)
        wide[:, :w] = pr.to_bf16_bits(X)
    else:
        wide = np.full((rows, ld), np.nan, dtype=np.float32)
        wide[:, :w] = X
    return wide[:, :w]
