"""EDGE GATV2 on the GPU (include/fora_hip_edge_gatv2.h): bits against the twin (tests/subgraph_gatv2_ref.py) and between calls."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import narrow_ref
import propagate_ref as pr
import subgraph_gatv2_ref as g2
import subgraph_prop_ref as sr
from test_subgraph_attention_bwd_gpu import _lens, _same
from test_subgraph_prop_gpu import _eq, _p, crafted  # noqa: F401  (crafted: the module-scoped fixture, an Engine of this module's own)

pytestmark = pytest.mark.gpu
E_ARG, SLOPE, DV = -1, 0.2, 8
# GV2_STAGE of fora_amd/csrc/fora_subgraph_gatv2.h is 512: a chunk of hc * d <= 512 elements has its group's row and att staged in
# LDS.  heads = 5 with d = 129 reads them in place for the chunk of four heads (516) and stages the ragged chunk of one (129).
SHAPES = [(1, 3), (1, 16), (1, 70), (5, 3), (5, 16), (5, 70), (5, 129)]


@functools.lru_cache(maxsize=None)
def _operands(heads, d):
    rng = np.random.Generator(np.random.PCG64(10700 + 1000 * heads + d))
    return tuple(rng.standard_normal(s).astype(np.float32) for s in ((sr.CRAFTED_NC, heads * d), (sr.CRAFTED_NC, heads * d), (heads, d), (sr.CRAFTED_NC, heads * DV)))


@functools.lru_cache(maxsize=None)
def _want(sub, by, heads, d):
    return g2.forward(sub.sub[0], sub.sub[1], *_operands(heads, d), heads=heads, slope=SLOPE, by=by)


def _fwd(eng, ops, want, by, heads, name, **kinds):
    o32, o64, y32, y64, st = eng.subgraph_gatv2(*ops, heads=heads, slope=SLOPE, by=by, want64=True, want_y32=True, want_y64=True, **kinds)
    for got, w, what in zip((o64, o32, y64, y32), want, ("out64", "out32", "y64", "y32")):
        _same(got, w, f"{what} {name}")
    return st


@pytest.mark.parametrize("short", [256, 64, 0])
@pytest.mark.parametrize("heads,d", SHAPES)
@pytest.mark.parametrize("by", ["row", "col"])
def test_one_call_against_the_twin(crafted, by, heads, d, short):
    lens = _lens(crafted, by)
    crafted.take()
    crafted.eng.set_option("attn_short", short)
    st = _fwd(crafted.eng, _operands(heads, d), _want(crafted, by, heads, d), by, heads, f"d={d}")
    assert (st["edges"], st["short_groups"], st["long_groups"], st["nan_pairs"]) == (lens.sum(), ((lens > 0) & (lens <= short)).sum(), (lens > short).sum(), 0)


@pytest.mark.parametrize("by", ["row", "col"])
def test_head_slices_narrow_types_and_non_finite_scores(crafted, by):
    eng, heads, d = crafted.eng, 5, 16
    xl, xr, att, V = _operands(heads, d)
    crafted.take()
    eng.set_option("attn_short", 64)                                                   # both paths
    _, o64, _, y64, _ = eng.subgraph_gatv2(xl, xr, att, V, heads=heads, slope=SLOPE, by=by, want32=False, want64=True, want_y64=True)
    for h in range(heads):                                                             # (slices read in place; row h of att a one-row operand)
        hs, vs = slice(h * d, (h + 1) * d), slice(h * DV, (h + 1) * DV)
        _, one, _, y, _ = eng.subgraph_gatv2(xl[:, hs], xr[:, hs], att[h:h + 1], V[:, vs], heads=1, slope=SLOPE, by=by, want32=False, want64=True, want_y64=True)
        _eq(one, np.ascontiguousarray(o64[:, vs]), f"out64 of head {h} alone")
        _eq(y[0], y64[h], f"y64 of head {h} alone")
    # ---- narrow types: bit for bit the call on the widened f32 operands
    heads, d, nc = 3, 16, sr.CRAFTED_NC
    rng = np.random.Generator(np.random.PCG64(10790))
    xl = pr.to_bf16_bits(rng.standard_normal((nc, heads * d)).astype(np.float32))
    xr, att, v = (narrow_ref.moderate_codes(rng, kind, shape) for kind, shape in ((narrow_ref.E4M3, (nc, heads * d)), (narrow_ref.F16, (heads, d)), (narrow_ref.E5M2, (nc, heads * DV))))
    kinds = ("bf16", narrow_ref.E4M3, narrow_ref.F16, narrow_ref.E5M2)
    wide = [sr.widen32(x, k) for x, k in zip((xl, xr, att, v), kinds)]
    (ro, rkw), (ao, _), (vo, vkw) = (narrow_ref.as_operand(k, x) for k, x in zip(kinds[1:], (xr, att, v)))
    crafted.take((None, 1, None))                                                      # both paths; the long one cut again, one segment a chunk
    eng.set_option("attn_short", 64)
    eng.set_option("softmax_short", 64)
    o32, o64, y32, y64, _ = eng.subgraph_gatv2(*wide, heads=heads, slope=SLOPE, by=by, want64=True, want_y32=True, want_y64=True)
    _fwd(eng, (xl, ro, ao, vo), (o64, o32, y64, y32), by, heads, "bf16 xl, e4m3 xr, f16 att, e5m2 v", xl_kind="bf16", xr_kind=rkw, v_kind=vkw)
    # ---- non-finite scores are written and counted as the twin has them
    heads, d, node0 = 3, 16, 1 if by == "row" else 11   # group node0 + k has sr.LENS[k] edges
    xl, xr, att, V = (x.copy() for x in _operands(heads, d))
    group, other = (xl, xr) if by == "row" else (xr, xl)           # the operand read at the group's node, and the one gathered at its ids
    other[21 + 650, 2 * d + 5] = np.nan                            # head 2 of the group of 700: a NaN at one of its ids (no other group reads this row)
    # a term of +inf: no product of two finite f32 values overflows f64, so the x of the pair is +inf itself and att positive
    group[node0 + sr.LENS.index(63), d + 7], att[1, 7] = np.inf, 1.5   # head 1 of the group of 63: every score +inf
    want = g2.forward(crafted.sub[0], crafted.sub[1], xl, xr, att, V, heads=heads, slope=SLOPE, by=by)
    crafted.take()                                                 # (attn_short 256: the fused kernel's NaN stores for 63, k_attn_nan_rows' for 700)
    assert _fwd(eng, (xl, xr, att, V), want, by, heads, "non-finite")["nan_pairs"] == 2   # (the whole arrays: the neighbours are bit-exact)


def test_refusals_write_nothing_and_the_call_leaves_the_state_alone(crafted):
    eng, lib = crafted.eng, crafted.eng._lib
    crafted.take()
    nc, edges, heads, d = sr.CRAFTED_NC, crafted.sub[1].size, 2, 3
    xl, xr, att, V = _operands(heads, d)
    wx, wv, y, out = heads * d, heads * DV, np.full(heads * edges, 0.5, dtype=np.float32), np.full((nc, heads * DV), np.nan, dtype=np.float32)
    base = dict(ctx=eng._ctx, xl=_p(xl), lt=0, ldxl=wx, xr=_p(xr), rt=0, ldxr=wx, att=_p(att), at=0, ldatt=d, v=_p(V), vt=0, ldv=wv, d=d, dv=DV, heads=heads, slope=SLOPE, fl=0,
                o32=_p(out), o64=None, ldo=wv, y32=_p(y), y64=None, ycap=y.size)
    raw = lambda **kw: lib.fora_hip_subgraph_gatv2(*{**base, **kw}.values(), None, None)
    for kw in (dict(d=0), dict(ldatt=d - 1), dict(ldxl=wx - 1), dict(slope=np.inf), dict(slope=np.nan), dict(fl=1), dict(o32=None), dict(ycap=y.size - 1), dict(at=3),
               dict(att=None), dict(ctx=None)):
        assert raw(**kw) == E_ARG, kw
    assert np.isnan(out).all() and (y == 0.5).all()
    gen, timing = eng.get_option("sparse_generation"), eng.timing()
    assert [raw(fl=f) for f in (0, 2)] == [0, 0] and not np.isnan(out).any()
    assert eng.get_option("sparse_generation") == gen and eng.timing() == timing and eng.held_cols == nc and eng.get_option("sub_edges") == edges


def test_device_tensors_and_autograd():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "subgraph_gatv2_device_child.py")], capture_output=True, text=True, timeout=600, cwd=os.path.dirname(here))
    assert r.returncode == 0 and "subgraph gatv2 device ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
