"""The twin of the SCORES (SDDMM) contract (tests/sddmm_ref.py) against yardsticks that are not the twin: exact integer dot
products, math.fsum with the textbook error bound of the stated order of additions, and the equivalence of a narrower lane
group that runs only its own steps of the tree.  No GPU."""
import math

import numpy as np

import propagate_ref as pr
import sddmm_ref as sr


def _pattern(rng, nq, n, max_len):
    lens = rng.integers(0, max_len + 1, size=nq)
    lens[0] = 0
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([np.sort(rng.choice(n, size=int(L), replace=False)) for L in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return row_ptr, ids


def test_integer_data_gives_the_exact_dot_products():
    rng = np.random.Generator(np.random.PCG64(8100))
    nq, n = 9, 40
    row_ptr, ids = _pattern(rng, nq, n, 12)
    rows = sr.entry_rows(row_ptr)
    for d in (1, 3, 64, 65, 200):
        A = rng.integers(-1000, 1001, size=(nq, d)).astype(np.float32)
        B = rng.integers(-1000, 1001, size=(n, d)).astype(np.float32)
        want = [sum(int(x) * int(y) for x, y in zip(A[i], B[v])) for i, v in zip(rows, ids)]      # python integers
        out64, out32 = sr.sddmm_ref(row_ptr, ids, A, B)
        assert out64.shape == (len(ids),) and [int(x) for x in out64] == want
        assert (out64 == np.array(want, dtype=np.float64)).all()
        assert (out32 == out64.astype(np.float32)).all()
        # bf16 operands: integers of at most 8 significant bits survive the truncation
        A8 = rng.integers(-128, 129, size=(nq, d)).astype(np.float32)
        B8 = rng.integers(-128, 129, size=(n, d)).astype(np.float32)
        want = [sum(int(x) * int(y) for x, y in zip(A8[i], B8[v])) for i, v in zip(rows, ids)]
        for a_bf16 in (False, True):
            for b_bf16 in (False, True):
                out64, _ = sr.sddmm_ref(row_ptr, ids, pr.to_bf16_bits(A8) if a_bf16 else A8, pr.to_bf16_bits(B8) if b_bf16 else B8,
                                        a_bf16=a_bf16, b_bf16=b_bf16)
                assert [int(x) for x in out64] == want, (d, a_bf16, b_bf16)


def test_random_data_is_within_the_bound_of_the_stated_order():
    """every product is exact; a score is the sum of d numbers through a chain of at most ceil(d / 64) additions (the first
    one, onto +0.0, is exact too, but the bound does not lean on that) and 6 tree steps, so by the textbook bound for any
    summation tree of that depth |score - exact| <= depth * u * sum |t_c| to first order, u = 2^-53 -- the test uses
    (ceil(d / 64) + 6) * 2^-53 * sum |t_c|, computed here from d, not tuned"""
    rng = np.random.Generator(np.random.PCG64(8200))
    nq, n = 7, 30
    row_ptr, ids = _pattern(rng, nq, n, 10)
    rows = sr.entry_rows(row_ptr)
    for d in (1, 5, 64, 100, 257, 1000):
        A, B = pr.scaled_features(rng, nq, d), pr.scaled_features(rng, n, d)
        out64, _ = sr.sddmm_ref(row_ptr, ids, A, B)
        worst = 0.0
        for e, (i, v) in enumerate(zip(rows, ids)):
            t = A[i].astype(np.float64) * B[v].astype(np.float64)
            exact, mass = math.fsum(t), math.fsum(np.abs(t))
            bound = (-(-d // 64) + 6) * 2.0 ** -53 * mass
            err = abs(float(out64[e]) - exact)
            worst = max(worst, err / bound if bound else 0.0)
            assert err <= bound, (d, e, err, bound)
        print(f"d={d}: worst error / bound = {worst:.3f}")


def test_a_narrower_group_gives_the_bits_of_64_lanes():
    rng = np.random.Generator(np.random.PCG64(8300))
    nq, n = 6, 25
    row_ptr, ids = _pattern(rng, nq, n, 9)
    for d in range(1, 71):
        A, B = pr.scaled_features(rng, nq, d), pr.scaled_features(rng, n, d)
        A[1, 0] = -0.0                                  # a product that is -0.0: q_0 = +0.0 + -0.0 = +0.0 either way
        full, _ = sr.sddmm_ref(row_ptr, ids, A, B, lanes=64)
        lanes = 1
        while lanes < min(d, 64):
            lanes *= 2
        while lanes <= 64:                              # the smallest group that holds d, and every wider one
            got, _ = sr.sddmm_ref(row_ptr, ids, A, B, lanes=lanes)
            assert (got.view(np.uint64) == full.view(np.uint64)).all(), (d, lanes)
            lanes *= 2
    assert not np.signbit(sr.tree_sum(np.full((1, 1), -0.0))).any()
