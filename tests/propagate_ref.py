"""The numpy twin of the PROPAGATE contract (include/fora_hip.h, fora_hip_sparse_propagate): out[i][c] = sum over the
entries e of row i of w_e * H[id_e][c], in the contract's order of operations -- entry by entry inside a segment of 256,
the segments' partial sums one after the other.  The loop runs over entries and is vectorised over columns only; nothing
here calls np.sum, np.dot or @, whose order of additions is not the contract's.  numpy's elementwise float64 multiply, add
and divide are single IEEE operations (no fused multiply-add)."""
import numpy as np

SEG = 256


def widen_bf16(bits):
    """bf16 bit patterns (uint16) as float32: bits << 16, exact"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def to_bf16_bits(x):
    """float32 -> bf16 bit patterns by truncation: test features only (any uint16 pattern is a legal input)"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def weights(fix):
    """w_e = ldexp((double)fix_e, -62): the u64 -> f64 cast rounds to nearest even, the scaling is exact"""
    return np.ldexp(np.asarray(fix, dtype=np.uint64).astype(np.float64), -62)


def row_terms(ids, fix, H64):
    """[len, d] the terms w_e * h of one row, each one IEEE multiply"""
    return weights(fix)[:, None] * H64[np.asarray(ids, dtype=np.int64)]


def sum_row(terms, seg=SEG):
    """the contract's sum of one row's terms ([len, d] float64): P_s from +0.0 in entry order, acc = P_0, acc = acc + P_s.
    seg=None: no segmentation, one left-to-right sum (what a row of at most `seg` entries is anyway)."""
    length, d = terms.shape
    step = length if seg is None else seg
    acc = None
    for s0 in range(0, length, max(step, 1)):
        part = np.zeros(d, dtype=np.float64)
        for e in range(s0, min(length, s0 + step)):
            part = part + terms[e]
        acc = part if acc is None else acc + part
    return np.zeros(d, dtype=np.float64) if acc is None else acc


def propagate_ref(row_ptr, ids, fix, H, normalize=False, bf16=False, seg=SEG):
    """(out64 [nq, d], out32 [nq, d]) of the rows (row_ptr, ids, fix) of a fetched sparse result and the features H
    ([n, d] float32, or uint16 bf16 bit patterns with bf16=True)."""
    H64 = (widen_bf16(H) if bf16 else np.asarray(H, dtype=np.float32)).astype(np.float64)
    nq, d = len(row_ptr) - 1, H64.shape[1]
    out = np.zeros((nq, d), dtype=np.float64)
    fix = np.asarray(fix, dtype=np.uint64)
    for i in range(nq):
        lo, hi = int(row_ptr[i]), int(row_ptr[i + 1])
        acc = sum_row(row_terms(ids[lo:hi], fix[lo:hi], H64), seg)
        if normalize:
            S = sum(int(x) for x in fix[lo:hi]) & ((1 << 64) - 1)
            if S:
                acc = acc / np.ldexp(np.float64(np.uint64(S)), -62)
        out[i] = acc
    with np.errstate(over="ignore"):
        return out, out.astype(np.float32)


def prop_stats_ref(row_ptr, d, elt):
    lens = np.diff(np.asarray(row_ptr, dtype=np.int64))
    return {"entries": int(lens.sum()), "segments": int(((lens + SEG - 1) // SEG).sum()), "max_row": int(lens.max()) if lens.size else 0,
            "feat_bytes": int(lens.sum()) * d * elt}


def scaled_features(rng, n, d):
    """normal values scaled by 2^k, k uniform in [-20, 20], float32: sums over them depend on the order of the additions"""
    k = rng.integers(-20, 21, size=(n, d))
    return np.ldexp(rng.standard_normal((n, d)), k).astype(np.float32)
