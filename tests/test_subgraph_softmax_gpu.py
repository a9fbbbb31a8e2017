"""EDGE SOFTMAX on the GPU, through the C ABI (the contract of include/fora_hip_edge_softmax.h): the softmax over the rows or the
columns of the held subgraph and its gradient are the numpy twin's (tests/subgraph_softmax_ref.py) bit for bit for every head
count, operand type and value of "softmax_short"; one call for all heads equals the per-head calls; NaN groups are written and
counted; the calls leave the held result and the subgraph as they were -- every comparison here is an equality of bits.  Memory
of another GPU needs a second device and is not exercised here."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import softmax_ref
import subgraph_prop_ref as sr
import subgraph_softmax_ref as sm
from test_subgraph_prop_gpu import _eq, _p, crafted  # noqa: F401  (crafted: the module-scoped fixture, an Engine of this module's own)

pytestmark = pytest.mark.gpu
E_ARG = -1
SCALE = 0.75
ROW0, COL0 = 1, 11                      # group ROW0 + k (by row) or COL0 + k (by column) has sr.LENS[k] edges


def _operands(edges, heads):
    """scores (float32 up to three heads, float64 above) and g in both types, normal numbers a few units wide"""
    rng = np.random.Generator(np.random.PCG64(9980 + heads))
    s, g = rng.standard_normal((heads, edges)) * 4.0, rng.standard_normal((heads, edges))
    return s.astype(np.float32 if heads <= 3 else np.float64), g.astype(np.float32), g


@functools.lru_cache(maxsize=None)
def _want(sub, by, heads):
    """the twin's forward pass and its backward pass for (y f32, g f64) and (y f64, g f32): once per (by, heads)"""
    sub_ptr, sub_col = sub.sub[0], sub.sub[1]
    s, g32, g64 = _operands(sub_col.size, heads)
    y64, y32, _ = sm.forward(sub_ptr, sub_col, s, SCALE, by)
    return y64, y32, sm.backward(sub_ptr, sub_col, y32, g64, SCALE, by), sm.backward(sub_ptr, sub_col, y64, g32, SCALE, by)


def _group(sub, by, length):
    """the places in sub_col of the crafted group of that many edges"""
    sub_ptr, sub_col = sub.sub[0], sub.sub[1]
    k = sr.LENS.index(length)
    return np.arange(sub_ptr[ROW0 + k], sub_ptr[ROW0 + k + 1]) if by == "row" else np.flatnonzero(sub_col == COL0 + k)


@pytest.mark.parametrize("short", [256, 64, 0])
@pytest.mark.parametrize("heads", [1, 3, 8])
@pytest.mark.parametrize("by", ["row", "col"])
def test_forward_and_backward_against_the_twin(crafted, by, heads, short):
    eng, (sub_ptr, sub_col, _, _) = crafted.eng, crafted.sub
    crafted.take()
    eng.set_option("softmax_short", short)
    s, g32, g64 = _operands(sub_col.size, heads)
    y64, y32, dx_a, dx_b = _want(crafted, by, heads)
    o32, o64, st = eng.subgraph_softmax(s, scale=SCALE, by=by, want64=True)
    _eq(o64, y64, "y64")
    _eq(o32, y32, "y32")
    ptr = sub_ptr if by == "row" else sr.transpose(sub_ptr, sub_col)[0]
    assert (st["edges"], st["long_groups"], st["nan_groups"]) == (sub_col.size, softmax_ref.softmax_stats_ref(ptr, short)["long_rows"], 0)
    assert st["built"] == (1 if by == "col" else 0)                                   # (the subgraph was taken again: the first call by column builds)
    _eq(eng.subgraph_softmax(s, scale=SCALE, by=by)[0], y32, "y32 alone")
    _eq(eng.subgraph_softmax(s, scale=SCALE, by=by, want32=False, want64=True)[1], y64, "y64 alone")
    for h in range(heads):
        _eq(eng.subgraph_softmax(s[h:h + 1], scale=SCALE, by=by, want32=False, want64=True)[1][0], y64[h], f"head {h} alone")
    d32, d64, st = eng.subgraph_softmax_bwd(y32, g64, scale=SCALE, by=by, want64=True)
    _eq(d64, dx_a[0], "dx64, y f32 and g f64")
    _eq(d32, dx_a[1], "dx32, y f32 and g f64")
    assert (st["long_groups"], st["nan_groups"], st["built"]) == (softmax_ref.softmax_stats_ref(ptr, short)["long_rows"], 0, 0)
    _eq(eng.subgraph_softmax_bwd(y64, g32, scale=SCALE, by=by)[0], dx_b[1], "dx32 alone, y f64 and g f32")
    _eq(eng.subgraph_softmax_bwd(y64, g32, scale=SCALE, by=by, want32=False, want64=True)[1], dx_b[0], "dx64 alone, y f64 and g f32")
    _eq(eng.subgraph_softmax_bwd(y64[-1:], g32[-1:], scale=SCALE, by=by, want32=False, want64=True)[1][0], dx_b[0][-1], "the last head alone")


@pytest.mark.parametrize("by", ["row", "col"])
def test_nan_groups_and_negative_zero(crafted, by):
    eng, (sub_ptr, sub_col, _, _) = crafted.eng, crafted.sub
    s, _, g64 = _operands(sub_col.size, 2)
    s, g64 = s.copy(), g64.copy()
    s[1, _group(crafted, by, 65)[64]] = np.nan                                       # one lane's second value; a long group under 64
    s[1, _group(crafted, by, 300)[299]] = np.inf                                     # the second segment of a long group
    s[1, _group(crafted, by, 63)] = -np.inf
    s[0, _group(crafted, by, 257)[:256]] = -np.inf                                   # a whole segment of -inf beside one value: no NaN group
    for length in (1, 63, 700):
        g64[:, _group(crafted, by, length)] = -0.0                                   # every t is -0.0: D is +0.0 only if the +0.0 are added
    want = sm.forward(sub_ptr, sub_col, s, SCALE, by)
    y = sm.forward(sub_ptr, sub_col, _operands(sub_col.size, 2)[0], SCALE, by)[0]    # (of the clean scores: every y above 0)
    want_dx = sm.backward(sub_ptr, sub_col, y, g64, SCALE, by)
    assert want[2] == 3 and np.isnan(want[0][1]).sum() == 65 + 300 + 63 and not np.isnan(want[0][0]).any()
    for short in (256, 64):
        crafted.take()
        eng.set_option("softmax_short", short)
        o32, o64, st = eng.subgraph_softmax(s, scale=SCALE, by=by, want64=True)
        _eq(o64, want[0], f"y64 under {short}")                                      # the quiet NaN's bits, and every other group untouched
        _eq(o32, want[1], f"y32 under {short}")
        assert st["nan_groups"] == 3
        d32, d64, _ = eng.subgraph_softmax_bwd(y, g64, scale=SCALE, by=by, want64=True)
        _eq(d64, want_dx[0], f"dx64 under {short}")
        _eq(d32, want_dx[1], f"dx32 under {short}")


def test_refusals_write_nothing_and_the_calls_leave_the_state_alone(crafted):
    eng, lib = crafted.eng, crafted.eng._lib
    row_ptr, cols, sub_ptr, sub_col, _, _ = eng.store_take_subgraph([0, 0], want_eid=True)
    heads = 2
    s, g32, _ = _operands(sub_col.size, heads)
    out = np.full(heads * sub_col.size, np.nan, dtype=np.float32)

    def raw(ctx=eng._ctx, x=s, st=0, hh=heads, scale=1.0, fl=0, o32=out, cap=out.size, bwd=None):
        tail = (hh, scale, fl, _p(o32), None, cap, None, None)
        return lib.fora_hip_subgraph_softmax_bwd(ctx, _p(x), st, _p(bwd[0]), bwd[1], *tail) if bwd else lib.fora_hip_subgraph_softmax(ctx, _p(x), st, *tail)

    raw_bwd = lambda g=g32, gt=0, **kw: raw(bwd=(g, gt), **kw)

    bad = (dict(st=1), dict(st=4), dict(hh=0), dict(fl=1), dict(fl=4), dict(scale=np.inf), dict(o32=None), dict(cap=out.size - 1), dict(x=None), dict(ctx=None))
    for kw in bad:
        assert raw(**kw) == E_ARG and raw_bwd(**kw) == E_ARG, kw
    assert raw_bwd(g=None) == E_ARG and raw_bwd(gt=1) == E_ARG and np.isnan(out).all()
    # ---- the calls leave the held result and both transpositions as they were; the first call by column builds the subgraph's
    G = np.ones((2, 3), dtype=np.float32)
    assert eng.sparse_propagate_t(row_ptr, G)[2]["built"] == 1
    e = int(row_ptr[-1])
    held = [np.zeros(e, np.int32), np.zeros(e, np.uint64), np.zeros(e, np.int32), np.zeros(e, np.uint64)]
    eng.sparse_fetch(held[0], None, held[1], cap=e)
    gen, timing = eng.get_option("sparse_generation"), eng.timing()
    assert raw() == 0 and not np.isnan(out).any() and raw_bwd() == 0
    assert eng.subgraph_softmax(s, by="col")[2]["built"] == 1 and eng.subgraph_softmax_bwd(s, g32, by="col")[2]["built"] == 0
    assert eng.get_option("sparse_generation") == gen and eng.timing() == timing and eng.held_cols == sr.CRAFTED_NC
    eng.sparse_fetch(held[2], None, held[3], cap=e)
    _eq(held[2], held[0], "held ids")
    _eq(held[3], held[1], "held words")
    assert eng.sparse_propagate_t(row_ptr, G)[2]["built"] == 0 and eng.subgraph_propagate_t(np.ones((sr.CRAFTED_NC, 1), np.float32))[2]["built"] == 0
    for a, b, name in zip(eng.subgraph_transpose_fetch(), sr.transpose(sub_ptr, sub_col), ("in_ptr", "in_row", "in_pos")):
        _eq(a, b, name)
    # ---- a subgraph of 0 edges (store row 1: two nodes): FORA_OK, nothing written; then no subgraph held
    crafted.take(row=1)
    out[:] = np.nan
    assert eng.get_option("sub_edges") == 0 and raw() == 0 and raw_bwd() == 0 and raw(fl=2) == 0 and np.isnan(out).all()
    o32, o64, st = eng.subgraph_softmax(np.zeros((heads, 0), np.float32), by="col", want64=True)
    assert o32.shape == o64.shape == (heads, 0) and st["edges"] == 0 and st["built"] == 0
    eng.store_take_compact([0, 0])
    assert raw() == E_ARG and raw_bwd() == E_ARG and np.isnan(out).all()
    with pytest.raises(Exception):
        eng.subgraph_softmax(s)


def test_device_tensors_autograd_and_attention():
    """the torch part in a child of its own (tests/subgraph_softmax_device_child.py): torch and the library on one HIP runtime"""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "subgraph_softmax_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0 and "subgraph softmax device ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
