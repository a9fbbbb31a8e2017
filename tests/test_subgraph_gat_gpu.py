"""EDGE GAT and EDGE GAT, BACKWARD on the GPU, through the C ABI (the contracts of include/fora_hip_edge_gat.h): one call over the
held subgraph is the numpy twin's (tests/subgraph_gat_ref.py: the existing twins chained through float64) bit for bit for every
head count, dv, operand type, type of y and value of "attn_short", "softmax_short" and "prop_segs"; one call for all heads equals
the per-head calls, a gradient alone equals itself among the three; a refusal writes nothing and the calls leave the held state as
it was -- every comparison here is an equality of bits unless a NaN is involved."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import narrow_ref
import propagate_ref as pr
import subgraph_gat_ref as gat
import subgraph_prop_ref as sr
from fora_amd import capi
from test_subgraph_attention_bwd_gpu import _lens, _same
from test_subgraph_prop_gpu import _eq, _p, crafted  # noqa: F401  (crafted: the module-scoped fixture, an Engine of this module's own)

pytestmark = pytest.mark.gpu
E_ARG, SLOPE = -1, 0.2
ROW0, COL0 = 1, 11                      # group ROW0 + k (by row) or COL0 + k (by column) has sr.LENS[k] edges
DVS = (8, 70)                           # V = 2; V = 1, a ragged chunk width and 70 x heads columns past one pass of the lanes
FWD, BWD = ("out64", "out32", "y64", "y32"), ("del64", "del32", "der64", "der32", "dv64", "dv32")


@functools.lru_cache(maxsize=None)
def _operands(heads, dv):
    rng = np.random.Generator(np.random.PCG64(10500 + 100 * heads + dv))
    return tuple(rng.standard_normal((sr.CRAFTED_NC, w)).astype(np.float32) for w in (heads, heads, heads * dv, heads * dv))   # el, er, V, G


@functools.lru_cache(maxsize=None)
def _want(sub, by, heads, dv):
    """(the forward twin's five results, {64: the backward twin's six on its y64, 32: on its y32})"""
    el, er, V, G = _operands(heads, dv)
    fwd = gat.forward(sub.sub[0], sub.sub[1], el, er, V, heads=heads, slope=SLOPE, by=by)
    return fwd, {bits: gat.backward(sub.sub[0], sub.sub[1], el, er, V, G, y, heads=heads, slope=SLOPE, by=by) for bits, y in ((64, fwd[2]), (32, fwd[3]))}


def _fwd(eng, ops, want, by, heads, name, **kinds):
    o32, o64, y32, y64, st = eng.subgraph_gat(*ops, heads=heads, slope=SLOPE, by=by, want64=True, want_y32=True, want_y64=True, **kinds)
    for got, w, what in zip((o64, o32, y64, y32), want, FWD):
        _same(got, w, f"{what} {name}")
    return st


def _bwd(eng, ops, y, want, by, heads, name, **kinds):
    *got, st = eng.subgraph_gat_bwd(*ops, y, heads=heads, slope=SLOPE, by=by, want64=True, **kinds)
    for i, what in enumerate(BWD):
        _same(got[i ^ 1], want[i], f"{what} {name}")                                   # (the call returns del32 before del64)
    return st


@pytest.mark.parametrize("short", [256, 64, 0])
@pytest.mark.parametrize("heads", [1, 3, 5])
@pytest.mark.parametrize("by", ["row", "col"])
def test_one_call_against_the_twin(crafted, by, heads, short):
    eng, lens, xlens = crafted.eng, _lens(crafted, by), _lens(crafted, "col" if by == "row" else "row")
    crafted.take()
    eng.set_option("attn_short", short)
    split = lambda n: (((n > 0) & (n <= short)).sum(), (n > short).sum())
    for dv in DVS:
        el, er, V, G = ops = _operands(heads, dv)
        fwd, bwd = _want(crafted, by, heads, dv)
        st = _fwd(eng, ops[:3], fwd, by, heads, f"dv={dv}")
        assert (st["edges"], st["short_groups"], st["long_groups"], st["nan_pairs"]) == (lens.sum(), *split(lens), 0)
        for bits, y in ((64, fwd[2]), (32, fwd[3])):
            st = _bwd(eng, ops, y, bwd[bits], by, heads, f"dv={dv} y{bits}")
            assert (st["edges"], st["short_groups"], st["long_groups"], st["across_short"], st["across_long"]) == (lens.sum(), *split(lens), *split(xlens))
        for n, grad in enumerate(("del", "der", "dv")):                                # each gradient alone, the others absent (y32)
            *got, st = eng.subgraph_gat_bwd(*ops, y, heads=heads, slope=SLOPE, by=by, **{f"want_{g}": g == grad for g in ("del", "der", "dv")})
            assert [o is not None for o in got] == [k == 2 * n for k in range(6)]
            _eq(got[2 * n], bwd[32][2 * n + 1], f"{grad}32 alone")
        for h in range(heads):                                                         # per-head calls on column slices (read in place)
            hs, vs = slice(h, h + 1), slice(h * dv, (h + 1) * dv)
            _, o64, _, y64, _ = eng.subgraph_gat(el[:, hs], er[:, hs], V[:, vs], heads=1, slope=SLOPE, by=by, want32=False, want64=True, want_y64=True)
            _eq(o64, np.ascontiguousarray(fwd[0][:, vs]), f"out64 of head {h} alone")
            _eq(y64[0], fwd[2][h], f"y64 of head {h} alone")
            *got, _ = eng.subgraph_gat_bwd(el[:, hs], er[:, hs], V[:, vs], G[:, vs], fwd[2][h:h + 1], heads=1, slope=SLOPE, by=by, want32=False, want64=True)
            for n, cs in enumerate((hs, hs, vs)):
                _eq(got[2 * n + 1], np.ascontiguousarray(bwd[64][2 * n][:, cs]), f"{BWD[2 * n]} of head {h} alone")


@pytest.mark.parametrize("by", ["row", "col"])
def test_narrow_types_and_the_options_of_the_long_path(crafted, by):
    eng, heads, dv, (sub_ptr, sub_col) = crafted.eng, 3, 5, crafted.sub[:2]
    rng = np.random.Generator(np.random.PCG64(10590))
    el, g = (pr.to_bf16_bits(rng.standard_normal((sr.CRAFTED_NC, w)).astype(np.float32)) for w in (heads, heads * dv))
    er, v = (narrow_ref.moderate_codes(rng, kind, (sr.CRAFTED_NC, w)) for kind, w in ((narrow_ref.F16, heads), (narrow_ref.E4M3, heads * dv)))
    kinds = dict(el_kind="bf16", er_kind=narrow_ref.F16, v_kind=narrow_ref.E4M3)
    fwd = gat.forward(sub_ptr, sub_col, el, er, v, heads=heads, slope=SLOPE, by=by, **kinds)
    bwd = gat.backward(sub_ptr, sub_col, el, er, v, g, fwd[3], heads=heads, slope=SLOPE, by=by, g_kind="bf16", **kinds)
    (ro, _), (vo, vkw) = narrow_ref.as_operand(narrow_ref.F16, er), narrow_ref.as_operand(narrow_ref.E4M3, v)
    crafted.take()
    _fwd(eng, (el, ro, vo), fwd, by, heads, "bf16 el, f16 er, e4m3 v", el_bf16=True, v_bf16=vkw)
    _bwd(eng, (el, ro, vo, g), fwd[3], bwd, by, heads, "bf16 el, f16 er, e4m3 v, bf16 g", el_bf16=True, v_bf16=vkw, g_bf16=True)
    # ---- the long path under other options: attn_short = 64 sends 65 .. 700 there, softmax_short cuts them again, one segment a chunk
    ops, (fwd, bwd) = _operands(heads, DVS[0]), _want(crafted, by, heads, DVS[0])
    crafted.take((None, 1, None))
    eng.set_option("attn_short", 64)
    eng.set_option("softmax_short", 64)
    # ---- and operands that are column slices of wider arrays
    wide = [np.concatenate([np.full((sr.CRAFTED_NC, 3), 9.0, np.float32), x, np.full((sr.CRAFTED_NC, 2), 9.0, np.float32)], axis=1) for x in ops]
    for o, name in ((ops, "softmax_short = 64, prop_segs = 1"), ([w[:, 3:3 + x.shape[1]] for w, x in zip(wide, ops)], "column slices")):
        _fwd(eng, o[:3], fwd, by, heads, name)
        _bwd(eng, o, fwd[3], bwd[32], by, heads, name)


@pytest.mark.parametrize("by", ["row", "col"])
def test_non_finite_scores_are_written_and_counted(crafted, by):
    eng, heads, dv, node0 = crafted.eng, 3, DVS[0], ROW0 if by == "row" else COL0
    el, er, V, _ = (x.copy() for x in _operands(heads, dv))
    group, other = (el, er) if by == "row" else (er, el)           # the operand read at the group's node, and the one at the other end
    node = lambda length: node0 + sr.LENS.index(length)
    group[node(1), 0] = -np.inf                                    # head 0 of the group of one edge: -inf only
    group[node(63), 1] = np.inf                                    # head 1 of the group of 63: a maximum of +inf
    other[21 + 650, 2] = np.nan                                    # head 2 of the group of 700: one NaN score (no other group reads this node's scalar)
    want = gat.forward(crafted.sub[0], crafted.sub[1], el, er, V, heads=heads, slope=SLOPE, by=by)
    assert want[4] == 3 and np.isnan(want[2]).sum() == 1 + 63 + 700 and np.isnan(want[0]).sum() == 3 * dv
    for short in (256, 0):                                         # the fused kernel's NaN stores, then k_attn_nan_rows'
        crafted.take()
        eng.set_option("attn_short", short)
        assert _fwd(eng, (el, er, V), want, by, heads, f"attn_short = {short}")["nan_pairs"] == 3   # (the whole arrays: the neighbours are bit-exact)


def test_refusals_write_nothing_and_the_calls_leave_the_state_alone(crafted):
    eng, lib = crafted.eng, crafted.eng._lib
    crafted.take()
    nc, edges, heads, dv = sr.CRAFTED_NC, crafted.sub[1].size, 2, DVS[0]
    el, er, V, G = _operands(heads, dv)
    wv, y = heads * dv, np.full(heads * edges, 0.5, dtype=np.float32)
    out, dl, dr = np.full((nc, wv), np.nan, dtype=np.float32), np.full((nc, heads), np.nan, dtype=np.float32), np.full((nc, heads), np.nan, dtype=np.float64)

    def raw(bwd, **kw):
        a = dict(ctx=eng._ctx, el=_p(el), lt=0, ldel=heads, er=_p(er), rt=0, lder=heads, v=_p(V), vt=0, ldv=wv)
        if bwd:
            a.update(g=_p(G), gt=0, ldg=wv, y=_p(y), yt=0, ycap=y.size)
        a.update(dv=dv, heads=heads, slope=SLOPE, fl=0)
        gr = capi.AttnGrads(dq32=dl.ctypes.data, dk64=dr.ctypes.data, lddq=kw.pop("lddq", heads), lddk=heads, lddv=wv)
        a.update(dict(gr=None if kw.pop("absent", False) else C.byref(gr)) if bwd else dict(o32=_p(out), o64=None, ldo=wv, y32=_p(y), y64=None, ycap=y.size))
        assert set(kw) <= set(a), kw
        a.update(kw)
        return (lib.fora_hip_subgraph_gat_bwd if bwd else lib.fora_hip_subgraph_gat)(*a.values(), None, None)

    both = (dict(lt=3), dict(vt=7), dict(dv=0), dict(heads=0), dict(ldel=heads - 1), dict(lder=heads - 1), dict(ldv=wv - 1), dict(fl=1), dict(fl=4), dict(slope=np.inf),
            dict(slope=np.nan), dict(ycap=y.size - 1), dict(er=None), dict(ctx=None))
    for bwd, more in ((False, (dict(ldo=wv - 1), dict(o32=None), dict(heads=8193, dv=8))), (True, (dict(gt=3), dict(yt=1), dict(ldg=wv - 1), dict(lddq=heads - 1), dict(absent=True), dict(g=None)))):
        for kw in both + more:
            assert raw(bwd, **kw) == E_ARG, (bwd, kw)
    assert np.isnan(out).all() and np.isnan(dl).all() and np.isnan(dr).all() and (y == 0.5).all()
    # ---- the calls leave the held subgraph, its transposition, the generation and the timing as they were
    tr = eng.subgraph_transpose_fetch()
    gen, timing = eng.get_option("sparse_generation"), eng.timing()
    assert [raw(b, fl=f) for b in (True, False) for f in (0, 2)] == [0] * 4 and not (np.isnan(out).any() or np.isnan(dl).any() or np.isnan(dr).any())
    assert eng.get_option("sparse_generation") == gen and eng.timing() == timing and eng.held_cols == nc and eng.get_option("sub_edges") == edges
    for a, b, c, name in zip(eng.subgraph_transpose_fetch(), tr, sr.transpose(crafted.sub[0], crafted.sub[1]), ("in_ptr", "in_row", "in_pos")):
        _eq(a, b, name)
        _eq(a, c, name + " against the twin")
    # ---- a subgraph of 0 edges (store row 1: two nodes): every output +0.0, nothing built; then no subgraph held
    crafted.take(row=1)
    for by in ("row", "col"):
        o32, _, y32, _, st = eng.subgraph_gat(el[:2], er[:2], V[:2], heads=heads, by=by, want_y32=True)
        *got, st2 = eng.subgraph_gat_bwd(el[:2], er[:2], V[:2], G[:2], y32, heads=heads, by=by, want64=True)
        assert all(o.shape[0] == 2 and not o.view(np.uint8).any() for o in (o32, *got)) and y32.shape == (heads, 0)
        assert (st["edges"], st["short_groups"], st["long_groups"], st["built"], st2["across_long"], st2["built"]) == (0, 0, 0, 0, 0, 0)
    eng.store_take_compact([0, 0])
    out[:] = np.nan
    assert raw(False) == E_ARG and raw(True) == E_ARG and np.isnan(out).all()


def test_device_tensors_and_autograd():
    """the torch part in a child of its own (tests/subgraph_gat_device_child.py): torch and the library on one HIP runtime"""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "subgraph_gat_device_child.py")], capture_output=True, text=True, timeout=600, cwd=os.path.dirname(here))
    assert r.returncode == 0 and "subgraph gat device ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
