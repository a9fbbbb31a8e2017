"""EDGE ATTENTION, BACKWARD on the GPU, through the C ABI (the contract of include/fora_hip_edge_attention_bwd.h): one call over
the held subgraph is the numpy twin's (tests/subgraph_attention_bwd_ref.py: the existing twins chained through float64) bit for bit
for every head count, shape, operand type, type of y and value of "attn_short", "softmax_short" and "prop_segs"; one call for all
heads equals the per-head calls, a gradient alone equals itself among the three; a refusal writes nothing and the call leaves the
held state as it was -- every comparison here is an equality of bits unless a NaN is involved."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import narrow_ref
import propagate_ref as pr
import subgraph_attention_bwd_ref as bw
import subgraph_attention_ref as at
import subgraph_prop_ref as sr
from fora_amd import capi
from test_subgraph_prop_gpu import _eq, _p, crafted  # noqa: F401  (crafted: the module-scoped fixture, an Engine of this module's own)

pytestmark = pytest.mark.gpu
E_ARG = -1
SCALE = 0.375
ROW0, COL0 = 1, 11                      # group ROW0 + k (by row) or COL0 + k (by column) has sr.LENS[k] edges
SHAPES = ((8, 8), (70, 5))              # (d, dv): V = 2 and one lane group of 8; V = 1, a ragged chunk width and a second pass of the lanes
NAMES = ("dq64", "dq32", "dk64", "dk32", "dv64", "dv32")


@functools.lru_cache(maxsize=None)
def _operands(heads, d, dv):
    rng = np.random.Generator(np.random.PCG64(10300 + 100 * heads + d))
    return tuple(rng.standard_normal((sr.CRAFTED_NC, heads * w)).astype(np.float32) for w in (d, d, dv, dv))   # Q, K, V, G


@functools.lru_cache(maxsize=None)
def _want(sub, by, heads, d, dv, y_bits):
    """(y, the twin's six gradients on it): y the forward twin's y64 or y32"""
    Q, K, V, G = _operands(heads, d, dv)
    y = at.attention(sub.sub[0], sub.sub[1], Q, K, V, heads=heads, scale=SCALE, by=by)[2 if y_bits == 64 else 3]
    return y, bw.backward(sub.sub[0], sub.sub[1], Q, K, V, G, y, heads=heads, scale=SCALE, by=by)


def _lens(sub, by):
    return np.diff(sub.sub[0]) if by == "row" else np.bincount(sub.sub[1], minlength=sr.CRAFTED_NC)


def _same(got, want, name):
    """equal bits; where the twin has a NaN, a NaN"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), name
    _eq(np.where(nan, 0, got), np.where(nan, 0, want), name)


def _check(eng, operands, y, want, by, heads, name, **kinds):
    """one call with all six outputs against the twin; returns the stats"""
    *got, st = eng.subgraph_attention_bwd(*operands, y, heads=heads, scale=SCALE, by=by, want64=True, **kinds)
    for i, what in enumerate(NAMES):
        _same(got[i ^ 1], want[i], f"{what} {name}")                                   # (the call returns dq32 before dq64)
    return st


@pytest.mark.parametrize("short", [256, 64, 0])
@pytest.mark.parametrize("heads", [1, 3, 5])
@pytest.mark.parametrize("by", ["row", "col"])
def test_one_call_against_the_twin(crafted, by, heads, short):
    eng, lens, xlens = crafted.eng, _lens(crafted, by), _lens(crafted, "col" if by == "row" else "row")
    crafted.take()
    eng.set_option("attn_short", short)
    split = lambda n: (((n > 0) & (n <= short)).sum(), (n > short).sum())
    for i, (d, dv) in enumerate(SHAPES):
        Q, K, V, G = ops = _operands(heads, d, dv)
        for j, bits in enumerate((64, 32)):
            y, want = _want(crafted, by, heads, d, dv, bits)
            st = _check(eng, ops, y, want, by, heads, f"d={d} y{bits}")
            assert (st["edges"], st["short_groups"], st["long_groups"], st["across_short"], st["across_long"]) == (lens.sum(), *split(lens), *split(xlens))
            assert st["built"] == (1 if i == 0 and j == 0 else 0)                      # (the subgraph was taken again: the first call transposes)
        for n, grad in enumerate(("dq", "dk", "dv")):                                  # each gradient alone, the others absent (y32)
            *got, st = eng.subgraph_attention_bwd(*ops, y, heads=heads, scale=SCALE, by=by, **{f"want_{g}": g == grad for g in ("dq", "dk", "dv")})
            assert [o is not None for o in got] == [k == 2 * n for k in range(6)] and (st["across_short"] + st["across_long"] > 0) == (grad != "dq")
            _eq(got[2 * n], want[2 * n + 1], f"{grad}32 alone")
        for h in range(heads):                                                         # per-head calls on column slices (read in place)
            qs, vs = slice(h * d, (h + 1) * d), slice(h * dv, (h + 1) * dv)
            *got, _ = eng.subgraph_attention_bwd(Q[:, qs], K[:, qs], V[:, vs], G[:, vs], y[h:h + 1], heads=1, scale=SCALE, by=by, want32=False, want64=True)
            for n, cs in enumerate((qs, qs, vs)):
                _eq(got[2 * n + 1], np.ascontiguousarray(want[2 * n][:, cs]), f"{NAMES[2 * n]} of head {h} alone")


@pytest.mark.parametrize("by", ["row", "col"])
def test_narrow_types_and_the_options_of_the_long_path(crafted, by):
    eng, heads, (d, dv) = crafted.eng, 3, SHAPES[0]
    sub_ptr, sub_col = crafted.sub[0], crafted.sub[1]
    rng = np.random.Generator(np.random.PCG64(10390))
    q, g = (pr.to_bf16_bits(rng.standard_normal((sr.CRAFTED_NC, heads * w)).astype(np.float32)) for w in (d, dv))
    k, v = (narrow_ref.moderate_codes(rng, kind, (sr.CRAFTED_NC, heads * w)) for kind, w in ((narrow_ref.F16, d), (narrow_ref.E4M3, dv)))
    kinds = dict(q_kind="bf16", k_kind=narrow_ref.F16, v_kind=narrow_ref.E4M3)
    y = at.attention(sub_ptr, sub_col, q, k, v, heads=heads, scale=SCALE, by=by, **kinds)[3]
    want = bw.backward(sub_ptr, sub_col, q, k, v, g, y, heads=heads, scale=SCALE, by=by, g_kind="bf16", **kinds)
    (ko, _), (vo, vkw) = narrow_ref.as_operand(narrow_ref.F16, k), narrow_ref.as_operand(narrow_ref.E4M3, v)
    crafted.take()
    _check(eng, (q, ko, vo, g), y, want, by, heads, "bf16 q, f16 k, e4m3 v, bf16 g", q_bf16=True, v_bf16=vkw, g_bf16=True)
    # ---- the long path under other options: attn_short = 64 sends 65 .. 700 there, softmax_short cuts them again, one segment a chunk
    ops, (y, want) = _operands(heads, d, dv), _want(crafted, by, heads, d, dv, 32)
    crafted.take((None, 1, None))
    eng.set_option("attn_short", 64)
    eng.set_option("softmax_short", 64)
    _check(eng, ops, y, want, by, heads, "softmax_short = 64, prop_segs = 1")
    # ---- operands that are column slices of wider arrays
    wide = [np.concatenate([np.full((sr.CRAFTED_NC, 3), 9.0, np.float32), x, np.full((sr.CRAFTED_NC, 2), 9.0, np.float32)], axis=1) for x in ops]
    _check(eng, [w[:, 3:3 + x.shape[1]] for w, x in zip(wide, ops)], y, want, by, heads, "column slices")


@pytest.mark.parametrize("by", ["row", "col"])
def test_a_nan_in_g_stays_where_the_twin_has_it(crafted, by):
    eng, heads, (d, dv) = crafted.eng, 3, SHAPES[0]
    Q, K, V, G = (x.copy() for x in _operands(heads, d, dv))
    G[(ROW0 if by == "row" else COL0) + sr.LENS.index(63), dv] = np.nan                # head 1 of the group of 63 edges: its dy, ds and dq
    y = _want(crafted, by, heads, d, dv, 64)[0]
    want = bw.backward(crafted.sub[0], crafted.sub[1], Q, K, V, G, y, heads=heads, scale=SCALE, by=by)
    assert np.isnan(want[0]).sum() == d and np.isnan(want[2]).any() and np.isnan(want[4]).any()   # dq: that group and head alone
    for short in (256, 0):
        crafted.take()
        eng.set_option("attn_short", short)
        _check(eng, (Q, K, V, G), y, want, by, heads, f"attn_short = {short}")


def test_refusals_write_nothing_and_the_call_leaves_the_state_alone(crafted):
    eng, lib = crafted.eng, crafted.eng._lib
    crafted.take()
    nc, edges, heads, (d, dv) = sr.CRAFTED_NC, crafted.sub[1].size, 2, SHAPES[0]
    Q, K, V, G = _operands(heads, d, dv)
    wq, wv, y = heads * d, heads * dv, np.full(heads * edges, 0.5, dtype=np.float32)
    dq, dk, dv_ = (np.full((nc, w), np.nan, dtype=t) for w, t in ((wq, np.float32), (wq, np.float64), (wv, np.float32)))

    def raw(absent=False, **kw):
        a = dict(ctx=eng._ctx, q=_p(Q), qt=0, ldq=wq, k=_p(K), kt=0, ldk=wq, v=_p(V), vt=0, ldv=wv, g=_p(G), gt=0, ldg=wv, y=_p(y), yt=0, ycap=y.size,
                 d=d, dv=dv, heads=heads, scale=1.0, fl=0, lddq=wq, lddk=wq, lddv=wv)
        assert set(kw) <= set(a)
        a.update(kw)
        gr = capi.AttnGrads(lddq=a.pop("lddq"), lddk=a.pop("lddk"), lddv=a.pop("lddv"))
        if not absent:
            gr.dq32, gr.dk64, gr.dv32 = dq.ctypes.data, dk.ctypes.data, dv_.ctypes.data
        return lib.fora_hip_subgraph_attention_bwd(*a.values(), C.byref(gr), None, None)

    bad = (dict(qt=3), dict(gt=7), dict(yt=1), dict(d=0), dict(dv=0), dict(heads=0), dict(ldq=wq - 1), dict(ldk=wq - 1), dict(ldv=wv - 1), dict(ldg=wv - 1),
           dict(lddq=wq - 1), dict(lddk=wq - 1), dict(lddv=wv - 1), dict(fl=1), dict(fl=4), dict(scale=np.inf), dict(scale=np.nan), dict(absent=True),
           dict(ycap=y.size - 1), dict(g=None), dict(ctx=None))
    for kw in bad:
        assert raw(**kw) == E_ARG, kw
    assert np.isnan(dq).all() and np.isnan(dk).all() and np.isnan(dv_).all()
    # ---- the call leaves the held subgraph, its transposition and the generation as they were
    tr = eng.subgraph_transpose_fetch()
    gen, timing = eng.get_option("sparse_generation"), eng.timing()
    assert raw() == 0 and raw(fl=2) == 0 and not (np.isnan(dq).any() or np.isnan(dk).any() or np.isnan(dv_).any())
    assert eng.subgraph_attention_bwd(Q, K, V, G, y.reshape(heads, edges), heads=heads)[6]["built"] == 0
    assert eng.get_option("sparse_generation") == gen and eng.timing() == timing and eng.held_cols == nc and eng.get_option("sub_edges") == edges
    for a, b, c, name in zip(eng.subgraph_transpose_fetch(), tr, sr.transpose(crafted.sub[0], crafted.sub[1]), ("in_ptr", "in_row", "in_pos")):
        _eq(a, b, name)
        _eq(a, c, name + " against the twin")
    # ---- a subgraph of 0 edges (store row 1: two nodes): every gradient +0.0, nothing built; then no subgraph held
    crafted.take(row=1)
    for by in ("row", "col"):
        *got, st = eng.subgraph_attention_bwd(Q[:2], K[:2], V[:2], G[:2], np.zeros((heads, 0), np.float32), heads=heads, by=by, want64=True)
        assert all(o.shape[0] == 2 and not o.view(np.uint8).any() for o in got) and (st["edges"], st["short_groups"], st["across_long"], st["built"]) == (0, 0, 0, 0)
    eng.store_take_compact([0, 0])
    dq[:] = np.nan
    assert raw() == E_ARG and np.isnan(dq).all()


def test_device_tensors_and_autograd():
    """the torch part in a child of its own (tests/subgraph_attention_bwd_device_child.py): torch and the library on one HIP runtime"""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "subgraph_attention_bwd_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0 and "subgraph attention bwd device ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
