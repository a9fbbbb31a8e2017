"""EDGE GATV2, BACKWARD on the GPU (include/fora_hip_edge_gatv2_bwd.h): bits against the twin (tests/subgraph_gatv2_bwd_ref.py) and
between calls, on the crafted subgraph -- 722 groups, so three d att tiles, with group lengths 0, 1, 63 .. 257, 300 and 700 on
both sides."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import narrow_ref
import propagate_ref as pr
import subgraph_gatv2_bwd_ref as g2b
import subgraph_gatv2_ref as g2
import subgraph_prop_ref as sr
from fora_amd import capi
from test_subgraph_attention_bwd_gpu import _lens, _same
from test_subgraph_prop_gpu import _eq, _p, crafted  # noqa: F401  (crafted: the module-scoped fixture, an Engine of this module's own)

pytestmark = pytest.mark.gpu
E_ARG, SLOPE, DV = -1, 0.2, 8
NAMES = ("dxl64", "dxl32", "dxr64", "dxr32", "datt64", "datt32", "dv64", "dv32")
WANTS = ("want_dxl", "want_dxr", "want_datt", "want_dv")
# a lane owns 8 columns of a chunk a pass (64 * 8 = 512): heads = 5 with d = 129 takes two passes for the chunk of four heads (516)
# and one for the ragged chunk of one; d = 70 gives a lane more than one column with a ragged tail; d = 3 leaves most lanes idle
SHAPES = [(1, 3), (1, 70), (5, 16), (5, 129)]


@functools.lru_cache(maxsize=None)
def _operands(heads, d):
    rng = np.random.Generator(np.random.PCG64(10900 + 1000 * heads + d))
    nc = sr.CRAFTED_NC
    return tuple(rng.standard_normal(s).astype(np.float32) for s in ((nc, heads * d), (nc, heads * d), (heads, d), (nc, heads * DV), (nc, heads * DV)))   # xl, xr, att, V, G


@functools.lru_cache(maxsize=None)
def _want(sub, by, heads, d):
    """(y64 of the forward twin, the backward twin's eight on it)"""
    ops = _operands(heads, d)
    y64 = g2.forward(sub.sub[0], sub.sub[1], *ops[:4], heads=heads, slope=SLOPE, by=by)[2]
    return y64, g2b.backward(sub.sub[0], sub.sub[1], *ops, y64, heads=heads, slope=SLOPE, by=by)


def _bwd(eng, ops, y, want, by, heads, name, **kw):
    *got, st = eng.subgraph_gatv2_bwd(*ops, y, heads=heads, slope=SLOPE, by=by, want64=True, **kw)
    for i, what in enumerate(NAMES):
        _same(got[i ^ 1], want[i], f"{what} {name}")                                   # (the call returns each f32 before its f64)
    return st


@pytest.mark.parametrize("short", [256, 64, 0])
@pytest.mark.parametrize("heads,d", SHAPES)
@pytest.mark.parametrize("by", ["row", "col"])
def test_one_call_against_the_twin(crafted, by, heads, d, short):
    lens, xlens = _lens(crafted, by), _lens(crafted, "col" if by == "row" else "row")
    crafted.take()
    crafted.eng.set_option("attn_short", short)
    y64, want = _want(crafted, by, heads, d)
    st = _bwd(crafted.eng, _operands(heads, d), y64, want, by, heads, f"d={d}")
    split = lambda n: (((n > 0) & (n <= short)).sum(), (n > short).sum())
    assert (st["edges"], st["short_groups"], st["long_groups"], st["across_short"], st["across_long"]) == (lens.sum(), *split(lens), *split(xlens))


@pytest.mark.parametrize("by", ["row", "col"])
def test_absent_gradients_f32_y_narrow_types_and_head_slices(crafted, by):
    eng, heads, d, (sub_ptr, sub_col) = crafted.eng, 5, 16, crafted.sub[:2]
    xl, xr, att, V, G = ops = _operands(heads, d)
    y64, want = _want(crafted, by, heads, d)
    crafted.take()
    eng.set_option("attn_short", 64)                                                   # both paths on both sides
    # ---- each gradient alone equals its bits from the full call; dv alone reads none of xl, xr and att (NaN in their place)
    nan = [np.full_like(x, np.nan) for x in (xl, xr, att)]
    for n, w in enumerate(WANTS):
        *got, _ = eng.subgraph_gatv2_bwd(*(nan if w == "want_dv" else ops[:3]), V, G, y64, heads=heads, slope=SLOPE, by=by, **{k: k == w for k in WANTS})
        assert [o is not None for o in got] == [k == 2 * n for k in range(8)]
        _eq(got[2 * n], want[2 * n + 1], f"{w} alone")
    # ---- an f32 y: the twin on the widened y32
    y32 = y64.astype(np.float32)
    _bwd(eng, ops, y32, g2b.backward(sub_ptr, sub_col, *ops, y32, heads=heads, slope=SLOPE, by=by), by, heads, "y32")
    # ---- head slices: heads calls with heads = 1 on column slices (read in place; row h of att a one-row operand)
    for h in range(heads):
        hs, vs = slice(h * d, (h + 1) * d), slice(h * DV, (h + 1) * DV)
        *got, _ = eng.subgraph_gatv2_bwd(xl[:, hs], xr[:, hs], att[h:h + 1], V[:, vs], G[:, vs], y64[h:h + 1], heads=1, slope=SLOPE, by=by, want32=False, want64=True)
        for n, w in enumerate((want[0][:, hs], want[2][:, hs], want[4][h:h + 1], want[6][:, vs])):
            _eq(got[2 * n + 1], np.ascontiguousarray(w), f"{NAMES[2 * n]} of head {h} alone")
    # ---- narrow types: bit for bit the call on the widened f32 operands
    heads, nc = 3, sr.CRAFTED_NC
    rng = np.random.Generator(np.random.PCG64(10990))
    xl, g = (pr.to_bf16_bits(rng.standard_normal((nc, heads * w)).astype(np.float32)) for w in (d, DV))
    xr, att, v = (narrow_ref.moderate_codes(rng, kind, shape) for kind, shape in ((narrow_ref.E4M3, (nc, heads * d)), (narrow_ref.F16, (heads, d)), (narrow_ref.E5M2, (nc, heads * DV))))
    kinds = ("bf16", narrow_ref.E4M3, narrow_ref.F16, narrow_ref.E5M2, "bf16")
    wide = [sr.widen32(x, k) for x, k in zip((xl, xr, att, v, g), kinds)]
    (ro, rkw), (ao, akw), (vo, vkw) = (narrow_ref.as_operand(k, x) for k, x in zip(kinds[1:4], (xr, att, v)))
    y = g2.forward(sub_ptr, sub_col, *wide[:4], heads=heads, slope=SLOPE, by=by)[3]
    *ref, _ = eng.subgraph_gatv2_bwd(*wide, y, heads=heads, slope=SLOPE, by=by, want64=True)
    _bwd(eng, (xl, ro, ao, vo, g), y, [ref[i ^ 1] for i in range(8)], by, heads, "bf16 xl, e4m3 xr, f16 att, e5m2 v, bf16 g", xl_kind="bf16", xr_kind=rkw, att_kind=akw,
         v_kind=vkw, g_kind="bf16")


def test_refusals_write_nothing_and_the_call_leaves_the_state_alone(crafted):
    eng, lib = crafted.eng, crafted.eng._lib
    crafted.take()
    nc, edges, heads, d = sr.CRAFTED_NC, crafted.sub[1].size, 2, 3
    xl, xr, att, V, G = _operands(heads, d)
    wx, wv, y = heads * d, heads * DV, np.full(heads * edges, 0.5, dtype=np.float32)
    dl, da = np.full((nc, wx), np.nan, dtype=np.float32), np.full((heads, d), np.nan, dtype=np.float64)
    gr = capi.AttnGrads(dq32=dl.ctypes.data, lddq=wx, lddk=wx, lddv=wv)
    base = dict(ctx=eng._ctx, xl=_p(xl), lt=0, ldxl=wx, xr=_p(xr), rt=0, ldxr=wx, att=_p(att), at=0, ldatt=d, v=_p(V), vt=0, ldv=wv, g=_p(G), gt=0, ldg=wv, y=_p(y), yt=0,
                ycap=y.size, d=d, dv=DV, heads=heads, slope=SLOPE, fl=0, gr=C.byref(gr), da32=None, da64=_p(da), lddatt=d)
    raw = lambda **kw: lib.fora_hip_subgraph_gatv2_bwd(*{**base, **kw}.values(), None, None)
    for kw in (dict(lddatt=d - 1), dict(gr=None, da64=None), dict(yt=1), dict(ycap=y.size - 1), dict(g=None), dict(ctx=None)):
        assert raw(**kw) == E_ARG, kw
    assert np.isnan(dl).all() and np.isnan(da).all()
    gen = eng.get_option("sparse_generation")
    assert [raw(fl=f) for f in (0, 2)] == [0, 0] and not (np.isnan(dl).any() or np.isnan(da).any())
    assert eng.get_option("sparse_generation") == gen and eng.held_cols == nc and eng.get_option("sub_edges") == edges


def test_device_tensors_and_autograd():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "subgraph_gatv2_bwd_device_child.py")], capture_output=True, text=True, timeout=600, cwd=os.path.dirname(here))
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "subgraph gatv2_bwd device ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
