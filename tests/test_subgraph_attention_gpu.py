"""EDGE ATTENTION on the GPU, through the C ABI (the contract of include/fora_hip_edge_attention.h): one call over the rows or the
columns of the held subgraph is the numpy twin's (tests/subgraph_attention_ref.py: the three twins chained through float64) bit for
bit for every head count, shape, operand type and value of "attn_short", "softmax_short" and "prop_segs"; one call for all heads
equals the per-head calls; NaN pairs are written and counted; a refusal writes nothing and the call leaves the held state as it
was -- every comparison here is an equality of bits."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import narrow_ref
import propagate_ref as pr
import subgraph_attention_ref as at
import subgraph_prop_ref as sr
from test_subgraph_prop_gpu import _eq, _p, crafted  # noqa: F401  (crafted: the module-scoped fixture, an Engine of this module's own)

pytestmark = pytest.mark.gpu
E_ARG = -1
SCALE = 0.375
ROW0, COL0 = 1, 11                      # group ROW0 + k (by row) or COL0 + k (by column) has sr.LENS[k] edges
SHAPES = ((8, 8), (70, 5))              # (d, dv): one lane group of 8; past one pass of the 64 lane sums with V = 1 and a ragged chunk width


@functools.lru_cache(maxsize=None)
def _operands(heads, d, dv):
    rng = np.random.Generator(np.random.PCG64(10100 + 100 * heads + d))
    return tuple(rng.standard_normal((sr.CRAFTED_NC, heads * w)).astype(np.float32) for w in (d, d, dv))


@functools.lru_cache(maxsize=None)
def _want(sub, by, heads, d, dv):
    return at.attention(sub.sub[0], sub.sub[1], *_operands(heads, d, dv), heads=heads, scale=SCALE, by=by)


def _lens(sub, by):
    return np.diff(sub.sub[0]) if by == "row" else np.bincount(sub.sub[1], minlength=sr.CRAFTED_NC)


def _check(eng, operands, want, by, heads, name, **kinds):
    """one call with all four outputs against the twin; returns the stats"""
    o32, o64, y32, y64, st = eng.subgraph_attention(*operands, heads=heads, scale=SCALE, by=by, want64=True, want_y32=True, want_y64=True, **kinds)
    for got, w, what in ((o64, want[0], "out64"), (o32, want[1], "out32"), (y64, want[2], "y64"), (y32, want[3], "y32")):
        _eq(got, w, f"{what} {name}")
    return st


@pytest.mark.parametrize("short", [256, 64, 0])
@pytest.mark.parametrize("heads", [1, 3, 5])
@pytest.mark.parametrize("by", ["row", "col"])
def test_one_call_against_the_twin(crafted, by, heads, short):
    eng, lens = crafted.eng, _lens(crafted, by)
    crafted.take()
    eng.set_option("attn_short", short)
    for i, (d, dv) in enumerate(SHAPES):
        Q, K, V = ops = _operands(heads, d, dv)
        want = _want(crafted, by, heads, d, dv)
        st = _check(eng, ops, want, by, heads, f"d={d}")
        assert (st["edges"], st["short_groups"], st["long_groups"], st["nan_pairs"]) == (lens.sum(), ((lens > 0) & (lens <= short)).sum(), (lens > short).sum(), 0)
        assert st["built"] == (1 if by == "col" and i == 0 else 0)                     # (the subgraph was taken again: the first call by column builds)
        _eq(eng.subgraph_attention(*ops, heads=heads, scale=SCALE, by=by)[0], want[1], "out32 alone")
        _eq(eng.subgraph_attention(*ops, heads=heads, scale=SCALE, by=by, want32=False, want64=True)[1], want[0], "out64 alone")
        _eq(eng.subgraph_attention(*ops, heads=heads, scale=SCALE, by=by, want_y32=True)[2], want[3], "y32 beside out32")
        for h in range(heads):                                                         # per-head calls on column slices (read in place)
            qs, vs = slice(h * d, (h + 1) * d), slice(h * dv, (h + 1) * dv)
            _, o64, _, y64, _ = eng.subgraph_attention(Q[:, qs], K[:, qs], V[:, vs], heads=1, scale=SCALE, by=by, want32=False, want64=True, want_y64=True)
            _eq(o64, np.ascontiguousarray(want[0][:, vs]), f"out64 of head {h} alone")
            _eq(y64[0], want[2][h], f"y64 of head {h} alone")


@pytest.mark.parametrize("by", ["row", "col"])
def test_narrow_types_and_the_options_of_the_long_path(crafted, by):
    eng, heads, (d, dv) = crafted.eng, 3, SHAPES[0]
    rng = np.random.Generator(np.random.PCG64(10190))
    q = pr.to_bf16_bits(rng.standard_normal((sr.CRAFTED_NC, heads * d)).astype(np.float32))
    k, v = (narrow_ref.moderate_codes(rng, kind, (sr.CRAFTED_NC, heads * w)) for kind, w in ((narrow_ref.F16, d), (narrow_ref.E4M3, dv)))
    want = at.attention(crafted.sub[0], crafted.sub[1], q, k, v, heads=heads, scale=SCALE, by=by, q_kind="bf16", k_kind=narrow_ref.F16, v_kind=narrow_ref.E4M3)
    (ko, _), (vo, vkw) = narrow_ref.as_operand(narrow_ref.F16, k), narrow_ref.as_operand(narrow_ref.E4M3, v)
    crafted.take()
    _check(eng, (q, ko, vo), want, by, heads, "bf16 q, f16 k, e4m3 v", q_bf16=True, v_bf16=vkw)
    # ---- the long path under other options: attn_short = 64 sends 65 .. 700 there, softmax_short cuts them again, one segment a chunk
    ops, want = _operands(heads, d, dv), _want(crafted, by, heads, d, dv)
    crafted.take((None, 1, None))
    eng.set_option("attn_short", 64)
    eng.set_option("softmax_short", 64)
    _check(eng, ops, want, by, heads, "softmax_short = 64, prop_segs = 1")
    # ---- operands that are column slices of wider arrays
    wide = [np.concatenate([np.full((sr.CRAFTED_NC, 3), 9.0, np.float32), x, np.full((sr.CRAFTED_NC, 2), 9.0, np.float32)], axis=1) for x in ops]
    _check(eng, [w[:, 3:3 + x.shape[1]] for w, x in zip(wide, ops)], want, by, heads, "column slices")


@pytest.mark.parametrize("by", ["row", "col"])
def test_nan_pairs_are_written_and_counted(crafted, by):
    eng, heads, (d, dv), node0 = crafted.eng, 3, SHAPES[0], ROW0 if by == "row" else COL0
    Q, K, V = (x.copy() for x in _operands(heads, d, dv))
    node = lambda length: node0 + sr.LENS.index(length)
    K[21, 0] = 1.0
    Q[node(1), 0] = -np.inf                                        # head 0 of the group of one edge (its id is node 21): -inf only
    Q[node(63), d] = np.inf                                        # head 1 of the group of 63: scores of +-inf, a maximum of +inf
    K[21 + 650, 2 * d + 1] = np.nan                                # head 2 of the group of 700: one NaN score (no other group reads this row of k)
    want = at.attention(crafted.sub[0], crafted.sub[1], Q, K, V, heads=heads, scale=SCALE, by=by)
    assert want[4] == 3 and np.isnan(want[2]).sum() == 1 + 63 + 700 and np.isnan(want[0]).sum() == 3 * dv
    for short in (256, 0):                                         # the fused kernel's NaN stores, then k_attn_nan_rows'
        crafted.take()
        eng.set_option("attn_short", short)
        assert _check(eng, (Q, K, V), want, by, heads, f"attn_short = {short}")["nan_pairs"] == 3   # (the whole arrays: the neighbours are bit-exact)


def test_refusals_write_nothing_and_the_call_leaves_the_state_alone(crafted):
    eng, lib = crafted.eng, crafted.eng._lib
    crafted.take()
    sub_ptr, sub_col = crafted.sub[0], crafted.sub[1]
    nc, edges, heads, (d, dv) = sr.CRAFTED_NC, crafted.sub[1].size, 2, SHAPES[0]
    Q, K, V = _operands(heads, d, dv)
    out, y = np.full((nc, heads * dv), np.nan, dtype=np.float32), np.full(heads * edges, np.nan, dtype=np.float64)

    def raw(ctx=eng._ctx, q=Q, qt=0, ldq=heads * d, ldo=heads * dv, dd=d, dvv=dv, hh=heads, scale=1.0, fl=0, o32=out, ycap=y.size):
        return lib.fora_hip_subgraph_attention(ctx, _p(q), qt, ldq, _p(K), 0, heads * d, _p(V), 0, heads * dv, dd, dvv, hh, scale, fl, _p(o32), None, ldo, None, _p(y), ycap, None, None)

    bad = (dict(qt=3), dict(qt=7), dict(dd=0), dict(dvv=0), dict(hh=0), dict(hh=8193, ldq=1 << 20), dict(ldq=heads * d - 1), dict(ldo=heads * dv - 1), dict(fl=1), dict(fl=4),
           dict(scale=np.inf), dict(scale=np.nan), dict(o32=None), dict(ycap=y.size - 1), dict(q=None), dict(ctx=None))
    for kw in bad:
        assert raw(**kw) == E_ARG, kw
    assert np.isnan(out).all() and np.isnan(y).all()
    # ---- the call leaves the held subgraph, its transposition and the generation as they were
    tr = eng.subgraph_transpose_fetch()
    gen, timing = eng.get_option("sparse_generation"), eng.timing()
    assert raw() == 0 and raw(fl=2) == 0 and not np.isnan(out).any() and not np.isnan(y).any()
    assert eng.subgraph_attention(Q, K, V, heads=heads, by="col")[4]["built"] == 0
    assert eng.get_option("sparse_generation") == gen and eng.timing() == timing and eng.held_cols == nc and eng.get_option("sub_edges") == edges
    for a, b, c, name in zip(eng.subgraph_transpose_fetch(), tr, sr.transpose(sub_ptr, sub_col), ("in_ptr", "in_row", "in_pos")):
        _eq(a, b, name)
        _eq(a, c, name + " against the twin")
    # ---- a subgraph of 0 edges (store row 1: two nodes): every output row +0.0, nothing built; then no subgraph held
    crafted.take(row=1)
    for by in ("row", "col"):
        o32 = np.full((2, heads * dv), np.nan, dtype=np.float32)
        _, _, y32, _, st = eng.subgraph_attention(Q[:2], K[:2], V[:2], heads=heads, by=by, out32=o32, want_y32=True)
        assert not o32.view(np.uint32).any() and y32.shape == (heads, 0) and (st["edges"], st["short_groups"], st["long_groups"], st["built"]) == (0, 0, 0, 0)
    eng.store_take_compact([0, 0])
    out[:] = np.nan
    assert raw() == E_ARG and np.isnan(out).all()


def test_device_tensors_and_autograd():
    """the torch part in a child of its own (tests/subgraph_attention_device_child.py): torch and the library on one HIP runtime"""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "subgraph_attention_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0 and "subgraph attention device ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
