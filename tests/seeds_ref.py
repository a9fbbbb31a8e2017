"""The SEED SETS contract of include/fora_hip.h in Python ints: the weights at 2^-62, the combine of single-source rows,
and a row's top-k.  Nothing here runs on the GPU or calls the library."""
import math

ONE = 1 << 62


def uniform_wfix(k):
    """weights == NULL: seed j of k gets floor(2^62 / k) + (j < 2^62 mod k); the sum is 2^62 exactly."""
    base, rem = divmod(ONE, k)
    return [base + (1 if j < rem else 0) for j in range(k)]


def weighted_wfix(weights):
    """Given weights: S added left to right in doubles, wfix_j = (uint64_t)ldexp(w_j / S, 62) (exact ldexp, flooring cast)."""
    S = 0.0
    for w in weights:
        w = float(w)
        if not math.isfinite(w) or w < 0:
            raise ValueError("bad weight")
        S += w
    if not (S > 0) or not math.isfinite(S):
        raise ValueError("zero sum")
    return [int(math.ldexp(float(w) / S, 62)) for w in weights]


def combine(rows, wfix):
    """row[v] = sum_j floor(wfix_j * x_j[v] / 2^62): every term floored on its own, the terms added as integers.  rows: one
    sequence of ints per seed of the set (the fora_hip_query_batch_fix row of that seed), in the set's order."""
    assert len(rows) == len(wfix) and rows
    out = [0] * len(rows[0])
    for x, w in zip(rows, wfix):
        for v, xv in enumerate(x):
            if xv:
                out[v] += (w * int(xv)) >> 62
    return out


def topk(row, k):
    """(ids, scores) of the k largest words: word descending, ties by ascending id, zeros never listed, padded with (0, 0.0);
    a score is the word * 2^-62."""
    order = sorted((v for v, x in enumerate(row) if x > 0), key=lambda v: (-row[v], v))[:k]
    pad = k - len(order)
    return order + [0] * pad, [math.ldexp(float(row[v]), -62) for v in order] + [0.0] * pad
