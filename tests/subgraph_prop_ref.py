"""The numpy twin of SUBGRAPH PRODUCTS (fora_hip_subgraph_propagate, fora_hip_subgraph_propagate_t,
fora_hip_subgraph_transpose_fetch; include/fora_hip_gnn.h): the sums of tests/propagate_values_ref.py over the CSR of the held
subgraph (sub_ptr, sub_col), with unit weights where the caller gives none, the narrow element types widened through
tests/narrow_ref.py, and the MEAN rule -- the finished f64 sum of a row divided once by the number of its terms, a row without
terms +0.0.  Nothing here calls np.sum, np.dot or @ on floating point values."""
import numpy as np

import narrow_ref
import propagate_ref as pr
import propagate_values_ref as pv


def widen32(X, kind=None):
    """the float32 matrix a call reads: kind None float32 as it is, "bf16" uint16 codes, or the codes of a kind of narrow_ref"""
    if kind is None:
        return np.ascontiguousarray(X, dtype=np.float32)
    if kind == "bf16":
        return pr.widen_bf16(X)
    return narrow_ref.widen(kind, X)


def _weights(values, edges):
    return np.ones(edges, dtype=np.float64) if values is None else np.asarray(values)


def _mean(out64, counts):
    out = out64.copy()
    nz = counts > 0
    with np.errstate(invalid="ignore", over="ignore"):
        out[nz] = out64[nz] / counts[nz].astype(np.float64)[:, None]
    return out, out.astype(np.float32)


def transpose(sub_ptr, sub_col):
    """(in_ptr int64 [nc + 1], in_row int32, in_pos int64): the edges stably sorted by target -- column by column the row an
    entry came from and its place in sub_col, ascending inside a column"""
    sub_ptr, sub_col = np.asarray(sub_ptr, dtype=np.int64), np.asarray(sub_col, dtype=np.int64)
    nc = sub_ptr.size - 1
    in_pos = np.argsort(sub_col, kind="stable").astype(np.int64)
    rows = np.repeat(np.arange(nc, dtype=np.int32), np.diff(sub_ptr))
    in_ptr = np.zeros(nc + 1, dtype=np.int64)
    np.cumsum(np.bincount(sub_col, minlength=nc), out=in_ptr[1:])
    return in_ptr, rows[in_pos].astype(np.int32), in_pos


def propagate(sub_ptr, sub_col, X, values=None, mean=False, kind=None):
    """(out64, out32) [nc, d]: out[j] = sum over the edges e of row j, in the order of sub_col, of w_e * X[sub_col[e]]"""
    sub_ptr = np.asarray(sub_ptr, dtype=np.int64)
    assert not (mean and values is not None)
    out64, out32 = pv.propagate_vals_ref(sub_ptr, sub_col, _weights(values, len(sub_col)), widen32(X, kind))
    return _mean(out64, np.diff(sub_ptr)) if mean else (out64, out32)


def propagate_t(sub_ptr, sub_col, G, values=None, mean=False, kind=None):
    """(out64, out32) [nc, d]: out[v] = sum over the edges e with sub_col[e] == v, in ascending e, of w_e * G[row of e]"""
    sub_ptr = np.asarray(sub_ptr, dtype=np.int64)
    nc = sub_ptr.size - 1
    assert not (mean and values is not None)
    out64, out32 = pv.propagate_t_vals_ref(sub_ptr, sub_col, _weights(values, len(sub_col)), widen32(G, kind), nc)
    return _mean(out64, np.bincount(np.asarray(sub_col, dtype=np.int64), minlength=nc)) if mean else (out64, out32)


LENS = [0, 1, 63, 64, 65, 255, 256, 257, 300, 700]
CRAFTED_N, CRAFTED_NC = 800, 722


def crafted_graph():
    """(row_ptr, col, U) of 800 nodes, U the first 722: inside U, row 1 + k and column 11 + k have LENS[k] edges each, through the
    700 filler nodes 21 .. 720 (a filler has at most 11 edges inside U as a row, 10 as a column); row 3 (63 edges) starts with a
    duplicate pair, node 21 has a self-loop, the nodes 0 and 721 have no edge at all -- empty leading and trailing rows and
    columns; every filler also points at a node outside U, and the nodes outside point into it: edges the subgraph drops"""
    H, C, F, NF = 1, 11, 21, 700
    adj = [[] for _ in range(CRAFTED_N)]
    for k, length in enumerate(LENS):
        adj[H + k] = [F + j for j in range(length)]
    adj[H + 2][1] = adj[H + 2][0]
    for j in range(NF):
        adj[F + j] = [750 + j % 7] + [C + k for k, length in enumerate(LENS) if j < length]
    adj[F].append(F)
    for v in range(CRAFTED_NC, CRAFTED_N):
        adj[v] = [v % 11, F + v % 13]
    row_ptr = np.concatenate([[0], np.cumsum([len(a) for a in adj])]).astype(np.int64)
    return row_ptr, np.array([t for a in adj for t in a], dtype=np.int32), np.arange(CRAFTED_NC, dtype=np.int32)


def mean_backward_operand(G, counts):
    """G' of torch_ops.subgraph_propagate(norm="mean")'s backward pass: float32(float64(G[j]) / float64(max(count_j, 1)))"""
    c = np.maximum(np.asarray(counts, dtype=np.int64), 1).astype(np.float64)
    return (np.asarray(G, dtype=np.float32).astype(np.float64) / c[:, None]).astype(np.float32)
