"""EDGE GATV2 and EDGE GATV2, BACKWARD at the edges the calls' own files leave out: every lane group of the score step (d of
1 .. 130) and of the dy step (dv of 1 .. 130), the staging bound of the forward kernels from both sides (hc * d of 512, 513 and
516, d of 513), every count of column slots of a lane of the backward pass, every vector width of the product step for every
element type with its tail, head counts of whole chunks and of three, slopes of either sign, zero and above one, att as a view, a
pre-activation of exactly +-0.0, non-finite values in the backward call, pitched outputs and the tiles of d att.  The rows are
the table of tests/subgraph_gatv2_cases.py, which tests/test_subgraph_gatv2_cases_cpu.py proves to reach those branches.  Every
comparison is an equality of bits with the numpy twins (tests/subgraph_gatv2_ref.py, tests/subgraph_gatv2_bwd_ref.py) on the
widened operands, by row and by column, on the fused path and on the long one; where a NaN is involved, a NaN exactly where the
twin has one."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import subgraph_attention_ref as at
import subgraph_gatv2_bwd_ref as g2b
import subgraph_gatv2_cases as gc
import subgraph_gatv2_ref as g2
import subgraph_prop_ref as sr
import subgraph_ref
from fora_amd import capi
from test_subgraph_attention_bwd_gpu import _lens, _same  # noqa: F401
from test_subgraph_fused_edges_gpu import COL0, KEYWORD, ROW0, _codes, _stats
from test_subgraph_prop_gpu import Crafted, _eq, _p, crafted  # noqa: F401  (crafted: the module-scoped fixture, an Engine of this module's own)

pytestmark = pytest.mark.gpu
FWD = ("out64", "out32", "y64", "y32")
BWD = ("dxl64", "dxl32", "dxr64", "dxr32", "datt64", "datt32", "dv64", "dv32")
KWS = ("xl_kind", "xr_kind", "att_kind", "v_kind", "g_kind")
F32S = (gc.F32,) * 5
PREFIXES = (1, 256, 257, 512, 513)      # the groups of the subgraphs whose d att has one tile, one whole, 256 + 1, two whole, 512 + 1


@functools.lru_cache(maxsize=None)
def _operands(case):
    """(the five operands dense, values or codes as the twins widen them; the same as the engine takes them -- v, g and att views
    into wider arrays of random elements where the row says so)"""
    rng = np.random.Generator(np.random.PCG64(11100 + gc.CASES.index(case)))
    dense, given = [], []
    for _, kind, rows, w, side, ld, off in gc.operands(case):
        wide = _codes(rng, kind, (rows or sr.CRAFTED_NC, ld))
        view = wide[:, off:off + side * w]
        dense.append(np.ascontiguousarray(view))
        given.append(view.view(np.float16) if kind == gc.F16 else view)
    return tuple(dense), tuple(given)


def _twins(ptr, col, ops, kinds, heads, slope, by, y=None):
    """(the forward twin's five results, the backward twin's eight on y -- the forward twin's y64 unless given)"""
    wide = [sr.widen32(x, kind) for x, kind in zip(ops, kinds)]
    fwd = g2.forward(ptr, col, *wide[:4], heads=heads, slope=slope, by=by)
    return fwd, g2b.backward(ptr, col, *wide, fwd[2] if y is None else y, heads=heads, slope=slope, by=by)


@functools.lru_cache(maxsize=None)
def _want(sub, case, by):
    return _twins(sub.sub[0], sub.sub[1], _operands(case)[0], case.kinds, case.heads, case.slope, by)


def _fwd(eng, given, kinds, want, by, heads, slope, name, same=_eq):
    """one forward call for all four outputs against the twin; returns the stats"""
    kw = {k: KEYWORD[kind] for k, kind in zip(KWS[:4], kinds)}
    o32, o64, y32, y64, st = eng.subgraph_gatv2(*given[:4], heads=heads, slope=slope, by=by, want64=True, want_y32=True, want_y64=True, **kw)
    for got, w, what in zip((o64, o32, y64, y32), want, FWD):
        same(got, w, f"{what} {name}")
    return st


def _bwd(eng, given, kinds, y, want, by, heads, slope, name, same=_eq):
    """one backward call for all eight outputs against the twin; returns the stats"""
    kw = {k: KEYWORD[kind] for k, kind in zip(KWS, kinds)}
    *got, st = eng.subgraph_gatv2_bwd(*given, y, heads=heads, slope=slope, by=by, want64=True, **kw)
    for i, what in enumerate(BWD):
        same(got[i ^ 1], want[i], f"{what} {name}")                                    # (the call returns the float32 of a pair first)
    return st


def _both_paths(sub, given, kinds, fwd, bwd, by, heads, slope, shorts=(256, 0), y=None, same=_eq):
    """the forward call (unless fwd is None) and the backward call on y (the twin's y64 unless given) under every value of shorts"""
    eng = sub.eng
    try:
        for short in shorts:
            sub.take()
            eng.set_option("attn_short", short)
            name = f"{by} attn_short={short}"
            st = None
            if fwd is not None:
                st = _fwd(eng, given, kinds, fwd, by, heads, slope, name, same)
                assert st["nan_pairs"] == 0, name
            st2 = _bwd(eng, given, kinds, fwd[2] if y is None else y, bwd, by, heads, slope, name, same)
            _stats(sub, by, short, st, st2)
    finally:
        eng.reset_options()


def _means_something(fwd, bwd, slope):
    """the twin's results are finite and not all zero, so the equality of bits says something"""
    assert fwd[4] == 0 and all(np.isfinite(w).all() for w in fwd[:4] + bwd) and fwd[0].any() and fwd[2].any()
    assert bwd[4].all() and bwd[6].any()                                               # every element of d att; dv
    assert slope == 0 or (bwd[0].any() and bwd[2].any())                               # (with a slope of 0 d xl and d xr may have zeros)


@pytest.mark.parametrize("by", ["row", "col"])
@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_forward_and_backward_on_every_row_of_the_table(crafted, case, by):
    fwd, bwd = _want(crafted, case, by)
    _means_something(fwd, bwd, case.slope)
    _both_paths(crafted, _operands(case)[1], case.kinds, fwd, bwd, by, case.heads, case.slope, case.shorts)


@pytest.mark.parametrize("by", ["row", "col"])
def test_eight_heads_in_one_call_equal_eight_calls_of_one_head(crafted, by):
    case = next(c for c in gc.CASES if c.name == "heads8")
    eng, heads, d, dv = crafted.eng, case.heads, case.d, case.dv
    (fwd, bwd), (_, given) = _want(crafted, case, by), _operands(case)
    crafted.take()
    for h in range(heads):                                                             # column slices, read in place; row h of att
        s1, vs, hh = slice(h * d, (h + 1) * d), slice(h * dv, (h + 1) * dv), slice(h, h + 1)
        ops = tuple(x[:, cs] for x, cs in zip(given, (s1, s1, slice(None), vs, vs)))
        ops = ops[:2] + (given[2][hh],) + ops[3:]
        one = tuple(np.ascontiguousarray(w[:, vs]) for w in fwd[:2]) + tuple(w[hh] for w in fwd[2:4])
        _fwd(eng, ops, F32S, one, by, 1, case.slope, f"head {h} alone")
        grads = tuple(np.ascontiguousarray(w[:, s1]) for w in bwd[:4]) + tuple(w[hh] for w in bwd[4:6]) + tuple(np.ascontiguousarray(w[:, vs]) for w in bwd[6:])
        _bwd(eng, ops, F32S, fwd[2][hh], grads, by, 1, case.slope, f"head {h} alone")


@pytest.mark.parametrize("by", ["row", "col"])
@pytest.mark.parametrize("name", ["lanes-d2", "slots-h4-d80", "stage-h4-d129", "heads9"])
def test_the_gradients_without_d_att_are_the_full_calls_bits_on_both_paths(crafted, name, by):
    """d att absent: the along pass keeps no sum of a (the short groups' kernel, and with "attn_short" 0 every group's segments);
    then the along gradient alone, without the across side"""
    case = next(c for c in gc.CASES if c.name == name)
    eng, (fwd, bwd), (_, given) = crafted.eng, _want(crafted, case, by), _operands(case)
    along = 0 if by == "row" else 2                                                    # d xl by row, d xr by column
    call = lambda **kw: eng.subgraph_gatv2_bwd(*given, fwd[2], heads=case.heads, slope=case.slope, by=by, want64=True, **kw)
    try:
        for short in (256, 0):
            crafted.take()
            eng.set_option("attn_short", short)
            *got, st = call(want_datt=False)
            assert got[4] is None and got[5] is None
            for i in (0, 1, 2, 3, 6, 7):
                _eq(got[i ^ 1], bwd[i], f"{BWD[i]} without d att, {by} attn_short={short}")
            _stats(crafted, by, short, None, st)
            *got, st = call(want_dxl=by == "row", want_dxr=by == "col", want_datt=False, want_dv=False)
            assert [o is not None for o in got] == [k in (along, along + 1) for k in range(8)]
            _eq(got[along + 1], bwd[along], f"{BWD[along]} alone, {by} attn_short={short}")
            _eq(got[along], bwd[along + 1], f"{BWD[along + 1]} alone, {by} attn_short={short}")
            assert (st["across_short"], st["across_long"]) == (0, 0)
    finally:
        eng.reset_options()


def _pre_activation(ptr, col, xl, xr, heads):
    """u [heads][edges, d] of the contract: xl at the edge's row plus xr at its column, in float64"""
    rows, cols, d = at.groups(ptr, col, "row"), np.asarray(col, dtype=np.int64), xl.shape[1] // heads
    with np.errstate(invalid="ignore"):
        return [xl.astype(np.float64)[rows, h * d:(h + 1) * d] + xr.astype(np.float64)[cols, h * d:(h + 1) * d] for h in range(heads)]


@pytest.mark.parametrize("by", ["row", "col"])
def test_a_pre_activation_of_exactly_zero_takes_att_not_att_times_slope(crafted, by):
    """u >= 0.0 from +-0.0 up: head 0 has one edge whose u are +0.0 (the self-loop, with xr = -xl on its columns), head 1 nothing
    but +0.0 (xl = c, xr = -c), head 2 nothing but -0.0.  Backward, such a column takes att itself, not att * slope"""
    heads, d, dv, (ptr, col) = 3, 8, 8, crafted.sub[:2]
    rng = np.random.Generator(np.random.PCG64(11190))
    xl, xr, att, V, G = (rng.standard_normal(s).astype(np.float32) for s in ((sr.CRAFTED_NC, heads * d),) * 2 + ((heads, d),) + ((sr.CRAFTED_NC, heads * dv),) * 2)
    xr[:, :d] = -xl[:, :d]
    xl[:, d:2 * d], xr[:, d:2 * d] = 0.625, -0.625
    xl[:, 2 * d:] = xr[:, 2 * d:] = -0.0
    u = _pre_activation(ptr, col, xl, xr, heads)
    loops = np.flatnonzero(at.groups(ptr, col, "row") == np.asarray(col)).tolist()
    assert len(loops) == 1 and np.flatnonzero((u[0] == 0).any(axis=1)).tolist() == loops and not u[0][loops[0]].any() and not np.signbit(u[0][loops[0]]).any()
    assert not u[1].any() and not np.signbit(u[1]).any() and not u[2].any() and np.signbit(u[2]).all()
    for slope in (0.2, -0.5):
        fwd, bwd = _twins(ptr, col, (xl, xr, att, V, G), F32S, heads, slope, by)
        assert fwd[4] == 0 and all(np.isfinite(w).all() for w in fwd[:4] + bwd) and all(w.any() for w in bwd[::2])
        assert bwd[0][:, d:2 * d].any() and bwd[2][:, d:2 * d].any()                  # the gradients of the head of zeros: ds * att
        _both_paths(crafted, (xl, xr, att, V, G), F32S, fwd, bwd, by, heads, slope)


@pytest.mark.parametrize("by", ["row", "col"])
@pytest.mark.parametrize("what,heads", [("nan-in-g", 11), ("nan-y", 32), ("nan-in-xl", 6)])
def test_non_finite_values_in_the_backward_call_stay_where_the_twin_has_them(crafted, what, heads, by):
    """nothing is checked, written in place of a result or counted: IEEE.  A NaN ds makes a whole row of d att NaN, and d att is
    [heads, d]: 11 heads keep one such row, 32 heads three, and 6 heads one element of it, under a tenth"""
    d, dv, slope, (ptr, col) = 2, 2, 0.2, crafted.sub[:2]
    node = (ROW0 if by == "row" else COL0) + sr.LENS.index(63)                         # the group of 63 edges
    rng = np.random.Generator(np.random.PCG64(11191))
    ops = tuple(rng.standard_normal(s).astype(np.float32) for s in ((sr.CRAFTED_NC, heads * d),) * 2 + ((heads, d),) + ((sr.CRAFTED_NC, heads * dv),) * 2)
    xl, xr, att, V, G = ops
    att[:3, 0] = np.abs(att[:3, 0])
    clean_y = g2.forward(ptr, col, *ops[:4], heads=heads, slope=slope, by=by)[2]
    assert np.isfinite(clean_y).all()

    def check(given, y, nans):
        with np.errstate(invalid="ignore"):
            want = g2b.backward(ptr, col, *given, y, heads=heads, slope=slope, by=by)
        assert all(np.isnan(w).mean() < 0.1 for w in want)                             # the equality of the rest means something
        assert [bool(np.isnan(w).any()) for w in want[::2]] == nans                    # d xl, d xr, d att, dv
        _both_paths(crafted, given, F32S, None, want, by, heads, slope, y=y, same=_same)
        return want
    if what == "nan-in-g":     # head 1 of the group of 63 edges: its dy, ds, du and a, and the rows of dv its y reaches
        Gn = G.copy()
        Gn[node, dv] = np.nan
        want = check((xl, xr, att, V, Gn), clean_y, [True, True, True, True])
        assert np.isnan(want[4][1]).all() and np.isnan(want[4]).sum() == d
    elif what == "nan-y":      # what the forward call wrote for a -inf-only, a +inf and a NaN head of that group
        xln, xrn = xl.copy(), xr.copy()
        grp = xln if by == "row" else xrn                                              # the operand read at the group's node
        grp[node, 0], grp[node, d], grp[node, 2 * d] = -np.inf, np.inf, np.nan         # (att[h, 0] > 0, slope > 0: every score of the head)
        with np.errstate(invalid="ignore", over="ignore"):
            y_nan, _, pairs = g2.forward(ptr, col, xln, xrn, att, V, heads=heads, slope=slope, by=by)[2:]
        assert pairs == 3 and np.isnan(y_nan).sum() == 3 * 63 and np.isnan(y_nan[:3]).sum() == 3 * 63
        check(ops, y_nan, [True, True, True, True])
    else:                      # u is NaN on the 63 edges of a row: w takes the multiplied branch and stays finite; a is NaN
        xln = xl.copy()
        xln[ROW0 + sr.LENS.index(63), d + 1] = np.nan
        assert [int(np.isnan(x).sum()) for x in _pre_activation(ptr, col, xln, xr, heads)[:3]] == [0, 63, 0]
        want = check((xln, xr, att, V, G), clean_y, [False, False, True, False])
        assert np.flatnonzero(np.isnan(want[4])).tolist() == [d + 1]
        clean = g2b.backward(ptr, col, *ops, clean_y, heads=heads, slope=slope, by=by)
        assert not np.array_equal(want[0], clean[0]) or not np.array_equal(want[2], clean[2])   # (some of those u were not negative)


def test_pitched_outputs_are_the_dense_calls_bits_and_leave_the_columns_behind_them(crafted):
    eng, lib, heads, d, dv, nc = crafted.eng, crafted.eng._lib, 3, 5, 6, sr.CRAFTED_NC
    rng = np.random.Generator(np.random.PCG64(11192))
    xl, xr, att, V, G = ops = tuple(rng.standard_normal(s).astype(np.float32) for s in ((nc, heads * d),) * 2 + ((heads, d),) + ((nc, heads * dv),) * 2)
    wx, wv, pad = heads * d, heads * dv, 7
    crafted.take()
    sevens = lambda rows, w, dtype: np.full((rows, w + pad), 7.0, dtype=dtype)

    def check(pairs, name):
        for (wide, w), dense, what in pairs:
            _eq(np.ascontiguousarray(wide[:, :w]), dense, f"{what} {name}")
            assert (wide[:, w:] == 7.0).all(), f"behind {what} {name}"
    for by in ("row", "col"):
        o32, o64, _, y64, _ = eng.subgraph_gatv2(*ops[:4], heads=heads, slope=gc.SLOPE, by=by, want64=True, want_y64=True)
        p32, p64 = sevens(nc, wv, np.float32), sevens(nc, wv, np.float64)
        eng.subgraph_gatv2(*ops[:4], heads=heads, slope=gc.SLOPE, by=by, out32=p32[:, :wv], out64=p64[:, :wv])
        check(zip(((p32, wv), (p64, wv)), (o32, o64), ("out32", "out64")), by)
        # ---- backward: the C entry point, every gradient a leading-column view of a wider array
        *dense, _ = eng.subgraph_gatv2_bwd(*ops, y64, heads=heads, slope=gc.SLOPE, by=by, want64=True)
        shapes = ((nc, wx), (nc, wx), (heads, d), (nc, wv))
        wide = [sevens(rows, w, t) for rows, w in shapes for t in (np.float32, np.float64)]
        lds = [w + pad for _, w in shapes]
        gr = capi.AttnGrads(dq32=wide[0].ctypes.data, dq64=wide[1].ctypes.data, lddq=lds[0], dk32=wide[2].ctypes.data, dk64=wide[3].ctypes.data, lddk=lds[1],
                            dv32=wide[6].ctypes.data, dv64=wide[7].ctypes.data, lddv=lds[3])
        rc = lib.fora_hip_subgraph_gatv2_bwd(eng._ctx, _p(xl), 0, wx, _p(xr), 0, wx, _p(att), 0, d, _p(V), 0, wv, _p(G), 0, wv, _p(y64), capi.PROP_F64, y64.size, d, dv, heads,
                                             gc.SLOPE, capi.SUB_BY_COL if by == "col" else 0, C.byref(gr), _p(wide[4]), _p(wide[5]), lds[2], None, None)
        assert rc == 0
        check(zip(zip(wide, (w for _, w in shapes for _ in range(2))), dense, (BWD[i ^ 1] for i in range(8))), by)


# ---- the tiles of d att: subgraphs of 1, 256, 257, 512 and 513 groups
class Prefixes(Crafted):
    """an Engine of its own over the crafted graph whose store holds, beside U, the prefixes U[:n] as further rows"""

    def __init__(self):
        import fora_amd
        self.row_ptr, self.col, self.U = sr.crafted_graph()
        self.eng = fora_amd.Engine(0)
        self.eng.set_graph(sr.CRAFTED_N, int(self.row_ptr[-1]), self.row_ptr, self.col)
        rows = [self.U] + [self.U[:n] for n in PREFIXES]
        ids = np.concatenate(rows).astype(np.int32)
        ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
        self.eng.store_load(ptr, ids, np.full(ids.size, 1 << 40, dtype=np.uint64))


@pytest.fixture(scope="module")
def prefixes():
    p = Prefixes()
    yield p
    p.eng.close()


@functools.lru_cache(maxsize=None)
def _prefix(n):
    """(the induced subgraph of U[:n], five float32 operands for heads 2, d 5, dv 8)"""
    row_ptr, col, U = sr.crafted_graph()
    rng = np.random.Generator(np.random.PCG64(11200 + n))
    return subgraph_ref.induced(row_ptr, col, U[:n]), tuple(rng.standard_normal(s).astype(np.float32) for s in ((n, 10), (n, 10), (2, 5), (n, 16), (n, 16)))


@pytest.mark.parametrize("by", ["row", "col"])
@pytest.mark.parametrize("n", PREFIXES)
def test_the_tiles_of_d_att_on_subgraphs_of_one_tile_whole_tiles_and_one_group_more(prefixes, n, by):
    heads, tile = 2, g2b.TILE
    tiles, last = -(-n // tile), n - (-(-n // tile) - 1) * tile
    assert (tiles, last) == {1: (1, 1), 256: (1, 256), 257: (2, 1), 512: (2, 256), 513: (3, 1)}[n] and tile == gc.GV2_TILE
    sub, ops = _prefix(n)
    k = 1 + PREFIXES.index(n)
    got = prefixes.take(row=k)
    assert prefixes.eng.held_cols == n and np.array_equal(got[2], sub[0]) and np.array_equal(got[3], sub[1])
    lens = np.diff(sub[0]) if by == "row" else np.bincount(sub[1], minlength=n)
    assert n == 1 or lens[n - 1] > 0                                                   # the one group of the last tile has edges
    fwd, bwd = _twins(sub[0], sub[1], ops, F32S, heads, gc.SLOPE, by)
    assert fwd[4] == 0 and all(np.isfinite(w).all() for w in fwd[:4] + bwd) and (n == 1 or bwd[4].all())
    holder = types.SimpleNamespace(eng=prefixes.eng, sub=sub, take=lambda: prefixes.take(row=k))
    _both_paths(holder, ops, F32S, fwd, bwd, by, heads, gc.SLOPE)
