"""Seed sets on CPU: the weight rules and the combine of tests/seeds_ref.py as the SEED SETS contract states them; the header
declares fora_hip_query_seeds_batch, the library exports it and fora_amd.capi binds it.  The GPU runs are in
test_seeds_gpu.py."""
import inspect
import os
import re

import pytest

import seeds_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fora_hip_query_seeds_batch"


@pytest.mark.parametrize("k", [1, 2, 3, 7, 1000])
def test_uniform_weights_sum_to_one_exactly(k):
    w = sr.uniform_wfix(k)
    assert len(w) == k and sum(w) == sr.ONE
    assert max(w) - min(w) <= 1 and w == sorted(w, reverse=True)  # the remainder goes to the first seeds
    if k == 3:
        assert sr.ONE % 3 != 0 and w[0] == w[2] + 1


EXACT = [[1.0], [0.5, 1.25, 2.0, 0.25], [3.0, 0.0, 1e-300], [7.0, 0.0, 0.0], [0.125] * 1024, [1.0, 3.0]]
ROUNDED = [[0.5, 1.25, 2.0, 0.75], [1e308, 1e307], [0.1] * 1000, [1.0, 1.0, 1.0]]


@pytest.mark.parametrize("weights", EXACT + ROUNDED)
def test_weighted_weights_stay_under_one(weights):
    """Each wfix <= 2^62.  Where S and the quotients w / S are exact in doubles (EXACT: dyadic weights with a power-of-two
    sum, or one weight that is the whole sum) the floors alone act and sum(wfix) <= 2^62, within the contract's 2^62 + k.
    Otherwise every add of S and every division rounds by up to 2^-53 relative, which is 2^9 units at 2^62 -- the
    contract's "up to the rounding of the k_g divisions": sum(wfix) <= 2^62 + 2^10 k ([0.1] * 1000 exceeds 2^62 + k)."""
    w = sr.weighted_wfix(weights)
    k = len(w)
    assert all(0 <= x <= sr.ONE for x in w)
    assert sum(w) <= sr.ONE + (k if weights in EXACT else 1024 * k)
    for x, y in zip(weights, w):
        if x == sum(weights):  # a weight equal to the whole sum
            assert y == sr.ONE
        if x == 0:
            assert y == 0


@pytest.mark.parametrize("bad", [[-1.0, 2.0], [float("nan")], [float("inf"), 1.0], [0.0, 0.0], [1e308, 1e308]])
def test_bad_weights_are_refused(bad):
    with pytest.raises(ValueError):
        sr.weighted_wfix(bad)


def test_singleton_is_the_identity():
    row = [0, 1, sr.ONE - 5, 12345678901234567, 3, 0, sr.ONE >> 1]
    assert sr.combine([row], sr.uniform_wfix(1)) == row
    assert sr.combine([row], sr.weighted_wfix([0.3])) == row
    whole = [0, sr.ONE, 0]  # the row of a dangling seed: exactly its weight, at the seed
    w = sr.uniform_wfix(3)
    assert sr.combine([whole, whole, [sr.ONE, 0, 0]], w) == [w[2], w[0] + w[1], 0]


def test_combine_floors_every_term_on_its_own():
    w = sr.uniform_wfix(3)
    assert sr.combine([[1], [1], [1]], w) == [0]  # three terms under one unit each: no mass is created
    assert sr.combine([[4], [4], [4]], w) == [3]  # floor(4/3 + ...) per term, not floor of the sum (4)
    ids, sc = sr.topk([0, 5, 9, 5, 0], 4)
    assert ids == [2, 1, 3, 0] and sc[:3] == [9 * 2.0 ** -62, 5 * 2.0 ** -62, 5 * 2.0 ** -62] and sc[3] == 0.0


def test_header_declares_the_entry_point_with_its_signature():
    hdr = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, "no declaration"
    args = [" ".join(re.sub(r"/\*.*?\*/", "", a, flags=re.S).split()) for a in m.group(1).split(",")]
    assert args == ["fora_ctx *ctx", "const int64_t *set_ptr", "const int32_t *seeds", "const double *weights", "int ns",
                    "int with_idx", "double *ppr_out", "uint64_t *ppr_fix_out", "int k", "int32_t *ids", "double *scores",
                    "uint64_t *row_sum_fix_out", "fora_seeds_stats *st"]
    assert " * SEED SETS (" in hdr and "} fora_seeds_stats;" in hdr


def test_capi_binds_it_and_the_engine_has_query_seeds():
    from fora_amd import capi
    assert NAME in capi.SYMBOLS
    sig = inspect.signature(capi.Engine.query_seeds)
    assert list(sig.parameters) == ["self", "sets", "weights", "with_idx", "k", "want_ppr", "want_fix"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["weights"], d["with_idx"], d["k"], d["want_ppr"], d["want_fix"]) == (None, False, 0, False, True)
    assert capi.STRUCTS["fora_seeds_stats"] is capi.SeedsStats  # (its fields and size against the header: tests/test_capi_cpu.py)


def test_library_exports_it_and_a_null_ctx_is_an_argument_error():
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    fn = getattr(capi.load(), NAME)
    assert fn(None, None, None, None, 0, 0, None, None, 0, None, None, None, None) == -1  # FORA_E_ARG, answered without a GPU
