"""The four fused calls on the held subgraph (EDGE ATTENTION, EDGE GAT and their backward calls) at the edges the family's own files
leave out: every lane group of the score step (d and dv of 1 .. 130), every vector width of the product step for every element type
with its tail, head counts of whole chunks, of three chunks and past the 64 heads a pass of k_sub_gat_across, scales and slopes of
either sign and zero, a pre-activation of exactly +-0.0 and non-finite values in EDGE GAT, BACKWARD.  The rows are the table of
tests/subgraph_fused_cases.py, which tests/test_subgraph_fused_cases_cpu.py proves to reach those branches.  Every comparison is
an equality of bits with the numpy twins (tests/subgraph_attention_ref.py, tests/subgraph_attention_bwd_ref.py,
tests/subgraph_gat_ref.py), by row and by column, on the fused path and on the long one; where a NaN is involved, a NaN exactly
where the twin has one."""
import functools

import numpy as np
import pytest

import narrow_ref
import propagate_ref as pr
import subgraph_attention_bwd_ref as bw
import subgraph_attention_ref as at
import subgraph_fused_cases as fc
import subgraph_gat_ref as gat
import subgraph_prop_ref as sr
from test_subgraph_attention_bwd_gpu import _lens, _same
from test_subgraph_prop_gpu import _eq, crafted  # noqa: F401  (crafted: the module-scoped fixture, an Engine of this module's own)

pytestmark = pytest.mark.gpu
ROW0, COL0 = 1, 11                      # group ROW0 + k (by row) or COL0 + k (by column) has sr.LENS[k] edges
KEYWORD = {fc.F32: False, fc.BF16: True, fc.F16: False, fc.E4M3: "e4m3", fc.E5M2: "e5m2"}   # beside the array (f16 by its dtype)
FWD = ("out64", "out32", "y64", "y32")
BWD = ("d1_64", "d1_32", "d2_64", "d2_32", "dv64", "dv32")       # d1, d2: dq and dk, or d el and d er
# the two calls of a family, the name of its parameter and the keywords of its four operands' types
CALLS = {"attn": ("subgraph_attention", "subgraph_attention_bwd", "scale", ("q_bf16", "k_bf16", "v_bf16", "g_bf16")),
         "gat": ("subgraph_gat", "subgraph_gat_bwd", "slope", ("el_bf16", "er_bf16", "v_bf16", "g_bf16"))}
F32S = (fc.F32,) * 4


def _codes(rng, kind, shape):
    if kind is fc.F32:
        return rng.standard_normal(shape).astype(np.float32)
    if kind == fc.BF16:
        return pr.to_bf16_bits(rng.standard_normal(shape).astype(np.float32))
    return narrow_ref.moderate_codes(rng, kind, shape).astype(narrow_ref.CODE_DTYPE[kind])


@functools.lru_cache(maxsize=None)
def _operands(case):
    """(the four operands as the twins take them -- dense arrays of values or codes, the same as the engine takes them -- v and g
    views into wider arrays of random elements where the row says so)"""
    rng = np.random.Generator(np.random.PCG64(10700 + fc.CASES.index(case)))
    dense, given = [], []
    for _, kind, w, ld, off in fc.operands(case):
        wide = _codes(rng, kind, (sr.CRAFTED_NC, ld))
        view = wide[:, off:off + case.heads * w]
        dense.append(np.ascontiguousarray(view))
        given.append(view.view(np.float16) if kind == fc.F16 else view)
    return tuple(dense), tuple(given)


def _twins(ptr, col, call, ops, kinds, heads, param, by, y=None):
    """(the forward twin's five results, the backward twin's six on y -- the forward twin's y64 unless given)"""
    a, b, v, g = ops
    ka, kb, kv, kg = kinds
    if call == "attn":
        fwd = at.attention(ptr, col, a, b, v, heads=heads, scale=param, by=by, q_kind=ka, k_kind=kb, v_kind=kv)
        return fwd, bw.backward(ptr, col, a, b, v, g, fwd[2] if y is None else y, heads=heads, scale=param, by=by, q_kind=ka, k_kind=kb, v_kind=kv, g_kind=kg)
    fwd = gat.forward(ptr, col, a, b, v, heads=heads, slope=param, by=by, el_kind=ka, er_kind=kb, v_kind=kv)
    return fwd, gat.backward(ptr, col, a, b, v, g, fwd[2] if y is None else y, heads=heads, slope=param, by=by, el_kind=ka, er_kind=kb, v_kind=kv, g_kind=kg)


@functools.lru_cache(maxsize=None)
def _want(sub, case, by):
    return _twins(sub.sub[0], sub.sub[1], case.call, _operands(case)[0], case.kinds, case.heads, case.param, by)


def _fwd(eng, call, given, kinds, want, by, heads, param, name, same=_eq):
    """one forward call for all four outputs against the twin; returns the stats"""
    fn, _, pname, kws = CALLS[call]
    kw = {k: KEYWORD[kind] for k, kind in zip(kws[:3], kinds)}
    o32, o64, y32, y64, st = getattr(eng, fn)(*given[:3], heads=heads, by=by, want64=True, want_y32=True, want_y64=True, **{pname: param}, **kw)
    for got, w, what in zip((o64, o32, y64, y32), want, FWD):
        same(got, w, f"{what} {name}")
    return st


def _bwd(eng, call, given, kinds, y, want, by, heads, param, name, same=_eq):
    """one backward call for all six outputs against the twin; returns the stats"""
    _, fn, pname, kws = CALLS[call]
    kw = {k: KEYWORD[kind] for k, kind in zip(kws, kinds)}
    *got, st = getattr(eng, fn)(*given, y, heads=heads, by=by, want64=True, **{pname: param}, **kw)
    for i, what in enumerate(BWD):
        same(got[i ^ 1], want[i], f"{what} {name}")                                    # (the calls return the float32 of a pair first)
    return st


def _stats(sub, by, short, fwd_st, bwd_st):
    lens, xlens = _lens(sub, by), _lens(sub, "col" if by == "row" else "row")
    split = lambda n: (((n > 0) & (n <= short)).sum(), (n > short).sum())
    if fwd_st is not None:
        assert (fwd_st["edges"], fwd_st["short_groups"], fwd_st["long_groups"]) == (lens.sum(), *split(lens)), (short, fwd_st)
    if bwd_st is not None:
        got = tuple(bwd_st[k] for k in ("edges", "short_groups", "long_groups", "across_short", "across_long"))
        assert got == (lens.sum(), *split(lens), *split(xlens)), (short, bwd_st)


def _both_paths(sub, call, given, kinds, fwd, bwd, by, heads, param, shorts=(256, 0), y=None, same=_eq, nan_pairs=0):
    """the forward call (unless fwd is None) and the backward call on y (the twin's y64 unless given) under every value of shorts"""
    eng = sub.eng
    try:
        for short in shorts:
            sub.take()
            eng.set_option("attn_short", short)
            name = f"{by} attn_short={short}"
            st = None
            if fwd is not None:
                st = _fwd(eng, call, given, kinds, fwd, by, heads, param, name, same)
                assert st["nan_pairs"] == nan_pairs, name
            st2 = _bwd(eng, call, given, kinds, fwd[2] if y is None else y, bwd, by, heads, param, name, same)
            _stats(sub, by, short, st, st2)
    finally:
        eng.reset_options()


def _row(sub, case, by):
    fwd, bwd = _want(sub, case, by)
    assert fwd[4] == 0 and all(np.isfinite(w).all() for w in fwd[:4] + bwd) and fwd[0].any() and bwd[4].any()
    assert case.param == 0 or (bwd[0].any() and bwd[2].any())                          # (a scale of 0 leaves no gradient of the scores)
    _both_paths(sub, case.call, _operands(case)[1], case.kinds, fwd, bwd, by, case.heads, case.param, case.shorts)


@pytest.mark.parametrize("by", ["row", "col"])
@pytest.mark.parametrize("case", fc.ATTN, ids=lambda c: c.name)
def test_attention_forward_and_backward_on_every_row_of_the_table(crafted, case, by):
    _row(crafted, case, by)


@pytest.mark.parametrize("by", ["row", "col"])
@pytest.mark.parametrize("case", fc.GAT, ids=lambda c: c.name)
def test_gat_forward_and_backward_on_every_row_of_the_table(crafted, case, by):
    _row(crafted, case, by)


@pytest.mark.parametrize("by", ["row", "col"])
@pytest.mark.parametrize("call", ["attn", "gat"])
def test_eight_heads_in_one_call_equal_eight_calls_of_one_head(crafted, call, by):
    case = next(c for c in fc.CASES if c.call == call and c.name == "heads8")
    eng, heads, d, dv = crafted.eng, case.heads, case.d, case.dv
    (fwd, bwd), (_, given) = _want(crafted, case, by), _operands(case)
    crafted.take()
    for h in range(heads):                                                             # column slices, read in place
        s1, vs = slice(h * d, (h + 1) * d), slice(h * dv, (h + 1) * dv)
        ops = tuple(x[:, cs] for x, cs in zip(given, (s1, s1, vs, vs)))
        one = tuple(np.ascontiguousarray(w[:, cs]) for w, cs in zip(fwd[:2], (vs, vs))) + tuple(w[h:h + 1] for w in fwd[2:4])
        _fwd(eng, call, ops, F32S, one, by, 1, case.param, f"head {h} alone")
        grads = tuple(np.ascontiguousarray(w[:, cs]) for w, cs in zip(bwd, (s1, s1, s1, s1, vs, vs)))
        _bwd(eng, call, ops, F32S, fwd[2][h:h + 1], grads, by, 1, case.param, f"head {h} alone")


@pytest.mark.parametrize("by", ["row", "col"])
def test_a_pre_activation_of_exactly_zero_is_passed_on_not_multiplied(crafted, by):
    """z >= 0.0 from +-0.0 up: head 0 has one z of +0.0 (the self-loop, with er = -el), head 1 nothing but +0.0 (el = c, er = -c),
    head 2 nothing but -0.0.  Backward, such an edge takes ds itself, not ds * slope"""
    heads, dv, (ptr, col) = 3, 8, crafted.sub[:2]
    rng = np.random.Generator(np.random.PCG64(10790))
    el, er, V, G = (rng.standard_normal((sr.CRAFTED_NC, w)).astype(np.float32) for w in (heads, heads, heads * dv, heads * dv))
    er[:, 0] = -el[:, 0]
    el[:, 1], er[:, 1] = 0.625, -0.625
    el[:, 2] = er[:, 2] = -0.0
    z = gat.pre_activation(ptr, col, el, er)
    loops = np.flatnonzero(at.groups(ptr, col, "row") == np.asarray(col)).tolist()
    assert len(loops) == 1 and np.flatnonzero(z[0] == 0).tolist() == loops and not np.signbit(z[0][loops[0]])
    assert not z[1].any() and not np.signbit(z[1]).any() and not z[2].any() and np.signbit(z[2]).all()
    for slope in (0.2, -0.5):
        fwd, bwd = _twins(ptr, col, "gat", (el, er, V, G), F32S, heads, slope, by)
        assert fwd[4] == 0 and all(w.any() for w in bwd[::2])
        _both_paths(crafted, "gat", (el, er, V, G), F32S, fwd, bwd, by, heads, slope)


@pytest.mark.parametrize("by", ["row", "col"])
def test_non_finite_values_in_the_gat_backward_stay_where_the_twin_has_them(crafted, by):
    heads, dv, slope, (ptr, col) = 3, 8, 0.2, crafted.sub[:2]
    node = lambda length: (ROW0 if by == "row" else COL0) + sr.LENS.index(length)
    rng = np.random.Generator(np.random.PCG64(10791))
    el, er, V, G = ops = tuple(rng.standard_normal((sr.CRAFTED_NC, w)).astype(np.float32) for w in (heads, heads, heads * dv, heads * dv))
    clean_fwd, clean = _twins(ptr, col, "gat", ops, F32S, heads, slope, by)
    few = lambda want: all(np.isnan(w).mean() < 0.1 for w in want)                     # the equality of the rest means something

    def check(given, y, nans):
        want = gat.backward(ptr, col, *given, y, heads=heads, slope=slope, by=by)
        assert few(want) and [bool(np.isnan(w).any()) for w in want[::2]] == nans
        _both_paths(crafted, "gat", given, F32S, None, want, by, heads, slope, y=y, same=_same)
        return want
    # ---- (a) a NaN in g: head 1 of the group of 63 edges -- its dy, ds and dz, and the rows of dv its y reaches
    Gn = G.copy()
    Gn[node(63), dv] = np.nan
    check((el, er, V, Gn), clean_fwd[2], [True, True, True])
    # ---- (b) a y with NaN rows: what the forward call wrote for a -inf-only, a +inf and a NaN (group, head)
    eln, ern = el.copy(), er.copy()
    grp = eln if by == "row" else ern                                                  # the operand read at the group's node
    grp[node(1), 0], grp[node(63), 1], grp[node(65), 2] = -np.inf, np.inf, np.nan
    y_nan, _, pairs = gat.forward(ptr, col, eln, ern, V, heads=heads, slope=slope, by=by)[2:]
    assert pairs == 3 and np.isnan(y_nan).sum() == 1 + 63 + 65
    check(ops, y_nan, [True, True, True])
    # ---- (c) a NaN in el: z is NaN on the 63 edges of a row, which take ds * slope -- nothing becomes NaN
    eln = el.copy()
    eln[ROW0 + sr.LENS.index(63), 1] = np.nan
    assert np.isnan(gat.pre_activation(ptr, col, eln, er)).sum() == 63
    want = check((eln, er, V, G), clean_fwd[2], [False, False, False])
    assert not np.array_equal(want[0], clean[0]) or not np.array_equal(want[2], clean[2])   # (some of those z were positive)
