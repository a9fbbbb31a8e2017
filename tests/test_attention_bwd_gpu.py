"""ATTENTION, BACKWARD (fora_hip_sparse_attention_bwd) on the GPU: dq, dk and dv of all heads in one call, bit for bit against the
numpy twin of the contract (tests/attention_bwd_ref.py) and against the five existing calls chained through float64 on the same
engine.  The held rows are attention_bwd_ref.injected(n): every boundary of the row side and of the column side.  Every
equality is on the bits of the float64 outputs; the float32 outputs are checked as (float) of them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import attention_bwd_ref as abr
import attention_ref as ar
import propagate_ref as pr
from fora_amd import capi
from test_sparse_gpu import SEED, _mixed_sources, _raw_fetch

pytestmark = pytest.mark.gpu

# (d, dv, heads, (q, k, v, g) as bf16, scale, (pitch padding, first column) of the wider arrays the operands are slices of, y as
# float64).  dv covers a lane group of one lane, a partial group, a full wave and a second column per lane of dy (130) and, as the
# width of dv's product, a tail lane behind vector loads; d the same for the products dq and dk (1, 3, 64, 65, 200).  The paddings
# make the pitches of cases 1 and 4 odd (one column per load) and keep those of cases 2, 3 and 5 multiples of a vector.
CASES = [
    (1, 1, 3, (False, False, False, False), 0.37, (0, 0), True),
    (3, 5, 2, (True, False, True, False), -2.0, (3, 1), False),
    (64, 64, 1, (False, True, False, True), 0.37, (4, 0), True),
    (65, 130, 1, (True, True, True, True), 0.0, (6, 0), False),
    (200, 5, 2, (False, False, True, False), 0.37, (1, 1), False),
    (64, 64, 3, (False, True, True, True), -2.0, (8, 0), True),
]
OPTIONS = (("prop_segs", 0), ("softmax_short", 256), ("attn_short", 256), ("propt_lds_cap", 4096))


def _load(engine, g, **kw):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(seed=SEED, epsilon=0.5, **kw)


def _slice(X, pad, off, bf16):
    """X as columns [off, off + w) of an array of w + pad + off columns whose other columns hold NaN patterns never to be read"""
    w = X.shape[1]
    return ar.padded(np.concatenate([np.zeros((X.shape[0], off), np.float32), X], axis=1), w + pad + off, bf16)[:, off:off + w]


def _operands(nq, n, d, dv, heads, bf16, pad=(0, 0), seed=9960):
    rng = np.random.Generator(np.random.PCG64(seed + 7 * d + dv))
    Q, K = ar.scores_operands(rng, nq, n, d, heads)
    V = (rng.standard_normal((n, heads * dv)) * np.exp2(rng.integers(-6, 7, size=(n, heads * dv)))).astype(np.float32)
    G = (rng.standard_normal((nq, heads * dv)) * np.exp2(rng.integers(-6, 7, size=(nq, heads * dv)))).astype(np.float32)
    return tuple(_slice(X, pad[0], pad[1], b) for X, b in zip((Q, K, V, G), bf16))


def _forward_y(engine, row_ptr, Q, K, V, heads, scale, bf16, y64):
    """y of the forward call on the same engine: ds gets both signs and a wide range from it"""
    r = engine.sparse_attention(row_ptr, Q, K, V, heads=heads, scale=scale, want32=True, want64=False, want_y32=not y64, want_y64=y64,
                                q_bf16=bf16[0], k_bf16=bf16[1], v_bf16=bf16[2])
    return r[3] if y64 else r[2]


@pytest.fixture(scope="module")
def held(engine_test, tiny):
    """the held result of the injected rows on the test build's engine, and the twins of the cases -- made once, never changed"""
    _load(engine_test, tiny)
    rows_fix = abr.injected(tiny.n)
    abr.check_injected(rows_fix)
    h = {"n": tiny.n, "nq": rows_fix.shape[0], "twin": {}}

    def hold():
        engine_test.sparse_clear()
        row_ptr, sp = engine_test.test_sparse_rows(rows_fix, threshold=0.0)
        assert (np.diff(row_ptr) == (rows_fix != 0).sum(axis=1)).all()
        e = int(row_ptr[-1])
        ids = np.zeros(e, np.int32)
        assert _raw_fetch(engine_test, ids, None, None, e) == 0
        h.update(row_ptr=row_ptr, ids=ids, entries=e)
    h["hold"] = hold
    hold()
    lens, cols = np.diff(h["row_ptr"]), np.bincount(h["ids"], minlength=tiny.n)
    h["empty_rows"], h["empty_cols"] = np.flatnonzero(lens == 0), np.flatnonzero(cols == 0)
    h["row_of_len"] = {int(L): int(np.flatnonzero(lens == L)[-1]) for L in (63, 600)}
    return h


def _reset(engine):
    engine.set_batch(0)
    for k, v in OPTIONS:
        if engine.get_option(k) != v:
            engine.set_option(k, v)


def _ensure_held(engine_test, tiny, held):
    """another module may have used the session's test engine in between: put graph and rows back if so"""
    e = held["entries"]
    ids = np.zeros(e, np.int32)
    if engine_test.n != tiny.n or _raw_fetch(engine_test, ids, None, None, e) != 0 or not (ids == held["ids"]).all():
        _load(engine_test, tiny)
        held["hold"]()
    _reset(engine_test)


def _twin(engine, held, case):
    if case not in held["twin"]:
        d, dv, heads, bf16, scale, pad, y64 = CASES[case]
        Q, K, V, G = _operands(held["nq"], held["n"], d, dv, heads, bf16, pad)
        y = _forward_y(engine, held["row_ptr"], Q, K, V, heads, scale, bf16, y64)
        assert y.dtype == (np.float64 if y64 else np.float32) and np.isfinite(y).all()
        held["twin"][case] = (Q, K, V, G, y, abr.attention_bwd_ref(held["row_ptr"], held["ids"], Q, K, V, G, y, held["n"], d, dv, heads, scale, *bf16))
    return held["twin"][case]


def _b64(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _b32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(got, want, what):
    """(dq32, dq64, dk32, dk64, dv32, dv64) of the engine against (dq64, dk64, dv64) of the twin"""
    for name, g32, g64, w64 in zip(("dq", "dk", "dv"), got[0::2], got[1::2], want):
        assert g64.shape == w64.shape and g32.shape == w64.shape, (what, name)
        assert (_b64(g64) == _b64(w64)).all(), (what, name, int((_b64(g64) != _b64(w64)).sum()))
        with np.errstate(over="ignore", invalid="ignore"):
            assert (_b32(g32) == _b32(g64.astype(np.float32))).all(), (what, name, "f32")


def _call(engine, row_ptr, Q, K, V, G, y, heads, scale, bf16, **kw):
    r = engine.sparse_attention_bwd(row_ptr, Q, K, V, G, y, heads=heads, scale=scale, want32=True, want64=True,
                                    q_bf16=bf16[0], k_bf16=bf16[1], v_bf16=bf16[2], g_bf16=bf16[3], **kw)
    return r[:6], r[6]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_equals_the_twin_on_both_paths(engine_test, tiny, held, case):
    _ensure_held(engine_test, tiny, held)
    d, dv, heads, bf16, scale, pad, y64 = CASES[case]
    Q, K, V, G, y, want = _twin(engine_test, held, case)
    assert all(np.isfinite(w).all() for w in want)
    if scale:                                                # ds has both signs
        assert (want[0] > 0).any() and (want[0] < 0).any()
    for short in (256, 0):
        engine_test.set_option("attn_short", short)
        got, st = _call(engine_test, held["row_ptr"], Q, K, V, G, y, heads, scale, bf16)
        _same(got, want, (CASES[case], short))
        ref = abr.attention_bwd_stats_ref(held["row_ptr"], held["ids"], held["n"], short)
        assert {k: st[k] for k in ref} == ref, (short, st)
        assert st["q_on_device"] == st["k_on_device"] == st["v_on_device"] == st["g_on_device"] == st["y_on_device"] == 0 and st["attn_ms"] >= 0.0
        # empty rows and empty columns: +0.0
        assert held["empty_rows"].size == 2 and (_b64(got[1][held["empty_rows"]]) == 0).all() and (_b32(got[0][held["empty_rows"]]) == 0).all()
        assert held["empty_cols"].size == 261
        for g32, g64 in ((got[2], got[3]), (got[4], got[5])):
            assert (_b64(g64[held["empty_cols"]]) == 0).all() and (_b32(g32[held["empty_cols"]]) == 0).all()
    engine_test.set_option("attn_short", 256)


@pytest.mark.parametrize("case", [1, 5])
def test_equals_the_five_calls_chained_through_f64(engine_test, tiny, held, case):
    _ensure_held(engine_test, tiny, held)
    d, dv, heads, bf16, scale, pad, y64 = CASES[case]
    Q, K, V, G, y, _ = _twin(engine_test, held, case)
    row_ptr = held["row_ptr"]
    for short in (256, 0):
        engine_test.set_option("attn_short", short)
        got, _ = _call(engine_test, row_ptr, Q, K, V, G, y, heads, scale, bf16)
        for j in range(heads):
            qs, vs = slice(j * d, (j + 1) * d), slice(j * dv, (j + 1) * dv)
            _, dy, _ = engine_test.sparse_sddmm(row_ptr, G[:, vs], V[:, vs], want32=False, want64=True, a_bf16=bf16[3], b_bf16=bf16[2])
            _, ds, _ = engine_test.sparse_softmax_bwd(row_ptr, np.ascontiguousarray(y[j]), dy, scale=scale, want32=False, want64=True)
            _, cq, _ = engine_test.sparse_propagate(row_ptr, K[:, qs], want32=False, want64=True, bf16=bf16[1], values=ds)
            _, ck, _ = engine_test.sparse_propagate_t(row_ptr, Q[:, qs], want32=False, want64=True, bf16=bf16[0], values=ds)
            _, cv, _ = engine_test.sparse_propagate_t(row_ptr, G[:, vs], want32=False, want64=True, bf16=bf16[3], values=np.ascontiguousarray(y[j]))
            assert (_b64(got[1][:, qs]) == _b64(cq)).all() and (_b64(got[3][:, qs]) == _b64(ck)).all() and (_b64(got[5][:, vs]) == _b64(cv)).all(), (case, short, j)
    engine_test.set_option("attn_short", 256)


def test_options_and_batch_change_no_bit(engine_test, tiny, held):
    _ensure_held(engine_test, tiny, held)
    case = 1
    d, dv, heads, bf16, scale, pad, y64 = CASES[case]
    Q, K, V, G, y, want = _twin(engine_test, held, case)
    try:
        for short, b, segs, sshort, lds in ((0, 0, 0, 256, 4096), (1, 1, 1, 0, 0), (64, 7, 3, 64, 64), (256, 0, 2, 1, 4096), (0, 2, 1, 0, 300)):
            engine_test.set_option("attn_short", short)
            engine_test.set_batch(b)
            engine_test.set_option("prop_segs", segs)
            engine_test.set_option("softmax_short", sshort)
            if engine_test.get_option("propt_lds_cap") != lds:
                engine_test.set_option("propt_lds_cap", lds)          # (the transposition is built again, on other tiers)
            got, st = _call(engine_test, held["row_ptr"], Q, K, V, G, y, heads, scale, bf16)
            _same(got, want, (short, b, segs, sshort, lds))
            ref = abr.attention_bwd_stats_ref(held["row_ptr"], held["ids"], held["n"], short)
            assert {k: st[k] for k in ref} == ref, (short, st)
        assert abr.attention_bwd_stats_ref(held["row_ptr"], held["ids"], held["n"], 1)["short_cols"] == 556
    finally:
        _reset(engine_test)


def test_the_column_plan_is_cached_with_the_transposition(engine_test, tiny, held):
    _ensure_held(engine_test, tiny, held)
    case = 1
    d, dv, heads, bf16, scale, pad, y64 = CASES[case]
    Q, K, V, G, y, want = _twin(engine_test, held, case)
    held["hold"]()                                            # a new held result: no transposition yet
    gen = engine_test.get_option("sparse_generation")
    first, st1 = _call(engine_test, held["row_ptr"], Q, K, V, G, y, heads, scale, bf16)
    assert st1["built"] == 1 and st1["plan_cached"] == 0 and st1["transpose_ms"] >= 0.0
    second, st2 = _call(engine_test, held["row_ptr"], Q, K, V, G, y, heads, scale, bf16)
    assert st2["built"] == 0 and st2["plan_cached"] == 1 and st2["transpose_ms"] == 0.0
    _same(first, want, "first")
    _same(second, want, "cached")
    engine_test.set_option("attn_short", 64)                  # another key: planned again, then cached again
    third, st3 = _call(engine_test, held["row_ptr"], Q, K, V, G, y, heads, scale, bf16)
    fourth, st4 = _call(engine_test, held["row_ptr"], Q, K, V, G, y, heads, scale, bf16)
    assert (st3["built"], st3["plan_cached"], st4["built"], st4["plan_cached"]) == (0, 0, 0, 1)
    _same(third, want, "attn_short 64")
    _same(fourth, want, "attn_short 64, cached")
    engine_test.set_option("attn_short", 256)
    # dq alone needs no transposition and no column plan
    _, _, _, _, _, _, st5 = engine_test.sparse_attention_bwd(held["row_ptr"], Q, K, V, G, y, heads=heads, scale=scale, want_dk=False, want_dv=False,
                                                            q_bf16=bf16[0], k_bf16=bf16[1], v_bf16=bf16[2], g_bf16=bf16[3])
    assert st5["built"] == 0 and st5["plan_cached"] == 0 and st5["columns"] == 0
    assert engine_test.get_option("sparse_generation") == gen                 # the held result was never touched
    # an existing transposed call reuses the transposition this call built
    _, _, pst = engine_test.sparse_propagate_t(held["row_ptr"], G[:, :dv], bf16=bf16[3], values=np.ascontiguousarray(y[0]))
    assert pst["built"] == 0
    held["hold"]()
    again, st6 = _call(engine_test, held["row_ptr"], Q, K, V, G, y, heads, scale, bf16)
    assert st6["built"] == 1 and st6["plan_cached"] == 0
    _same(again, want, "after a new hold")


def test_each_gradient_alone(engine_test, tiny, held):
    """one gradient at a time, into a column slice of a wider array: it equals its part of the full call, the columns beside it
    keep their sentinel, and the other two are not made"""
    _ensure_held(engine_test, tiny, held)
    case = 4
    d, dv, heads, bf16, scale, pad, y64 = CASES[case]
    Q, K, V, G, y, want = _twin(engine_test, held, case)
    nq, n = held["nq"], held["n"]
    kw = dict(heads=heads, scale=scale, q_bf16=bf16[0], k_bf16=bf16[1], v_bf16=bf16[2], g_bf16=bf16[3])
    for short in (256, 0):
        engine_test.set_option("attn_short", short)
        for i, (name, rows, w) in enumerate((("dq", nq, heads * d), ("dk", n, heads * d), ("dv", n, heads * dv))):
            w32, w64 = np.full((rows, w + 5), -7.0, np.float32), np.full((rows, w + 5), -7.0, np.float64)
            outs = {name + "32": w32[:, 2:2 + w], name + "64": w64[:, 2:2 + w]}
            r = engine_test.sparse_attention_bwd(held["row_ptr"], Q, K, V, G, y, want_dq=False, want_dk=False, want_dv=False, **outs, **kw)
            assert [x is None for x in r[:6]] == [k // 2 != i for k in range(6)], name
            assert (_b64(w64[:, 2:2 + w]) == _b64(want[i])).all() and (_b32(w32[:, 2:2 + w]) == _b32(want[i].astype(np.float32))).all(), (name, short)
            assert (w32[:, :2] == -7.0).all() and (w32[:, 2 + w:] == -7.0).all() and (w64[:, :2] == -7.0).all() and (w64[:, 2 + w:] == -7.0).all(), name
        # float32 only and float64 only
        r = engine_test.sparse_attention_bwd(held["row_ptr"], Q, K, V, G, y, want32=False, want64=True, want_dk=False, **kw)
        assert r[0] is None and r[2] is None and r[3] is None and r[4] is None and (_b64(r[1]) == _b64(want[0])).all() and (_b64(r[5]) == _b64(want[2])).all()
    engine_test.set_option("attn_short", 256)


def test_a_held_result_with_no_entries_writes_zeros(engine_test, tiny, held):
    _ensure_held(engine_test, tiny, held)
    n, nq, d, dv, heads = tiny.n, 3, 4, 3, 2
    try:
        row_ptr, _ = engine_test.test_sparse_rows(np.zeros((nq, n), np.uint64), threshold=0.0)
        assert int(row_ptr[-1]) == 0
        Q, K, V, G = _operands(nq, n, d, dv, heads, (False,) * 4)
        outs = {k: np.full((rows, w), -7.0, t) for k, rows, w, t in (("dq32", nq, heads * d, np.float32), ("dq64", nq, heads * d, np.float64),
                                                                       ("dk32", n, heads * d, np.float32), ("dk64", n, heads * d, np.float64),
                                                                       ("dv32", n, heads * dv, np.float32), ("dv64", n, heads * dv, np.float64))}
        for short in (256, 0):
            engine_test.set_option("attn_short", short)
            for o in outs.values():
                o[:] = -7.0
            r = engine_test.sparse_attention_bwd(row_ptr, Q, K, V, G, np.zeros((heads, 0), np.float32), heads=heads, **outs)
            assert r[6]["entries"] == 0 and r[6]["columns"] == 0
            for k, o in outs.items():
                assert (o.view(np.uint32 if k.endswith("32") else np.uint64) == 0).all(), (k, short)
    finally:
        held["hold"]()
        _reset(engine_test)


def test_nan_and_inf_in_y_follow_ieee_on_both_paths(engine_test, tiny, held):
    """a NaN in a short row of y and a +inf in a long one: the NaN-ness of every output equals the twin's, and every element the
    twin keeps finite has its bits"""
    _ensure_held(engine_test, tiny, held)
    case = 1
    d, dv, heads, bf16, scale, pad, y64 = CASES[case]
    Q, K, V, G, y, clean = _twin(engine_test, held, case)
    row_ptr = held["row_ptr"]
    for dtype in (np.float32, np.float64):
        yb = y.astype(dtype).copy()
        yb[0, row_ptr[held["row_of_len"][63]] + 40] = np.nan
        yb[1, row_ptr[held["row_of_len"][600]] + 599] = np.inf
        want = abr.attention_bwd_ref(row_ptr, held["ids"], Q, K, V, G, yb, held["n"], d, dv, heads, scale, *bf16)
        assert all(np.isnan(w).any() for w in want) and all(np.isfinite(w).any() for w in want)
        for short in (256, 0, 64):
            engine_test.set_option("attn_short", short)
            got, _ = _call(engine_test, row_ptr, Q, K, V, G, yb, heads, scale, bf16)
            for name, g32, g64, w64 in zip(("dq", "dk", "dv"), got[0::2], got[1::2], want):
                assert (np.isnan(g64) == np.isnan(w64)).all(), (name, short)
                fin = np.isfinite(w64)
                assert (_b64(g64[fin]) == _b64(w64[fin])).all(), (name, short)
                assert (np.isinf(g64) == np.isinf(w64)).all() and (g64[np.isinf(w64)] == w64[np.isinf(w64)]).all(), (name, short)
                with np.errstate(over="ignore", invalid="ignore"):
                    assert (_b32(g32[fin]) == _b32(g64[fin].astype(np.float32))).all() and (np.isnan(g32) == np.isnan(g64)).all(), (name, short)
    engine_test.set_option("attn_short", 256)


def _check_held(engine, row_ptr, ids, n, seed):
    d, dv, heads = 8, 6, 2
    nq = len(row_ptr) - 1
    for bf16, scale, y64 in (((False,) * 4, None, False), ((True,) * 4, -2.0, True)):
        Q, K, V, G = _operands(nq, n, d, dv, heads, bf16, seed=seed)
        sc = float(d) ** -0.5 if scale is None else scale
        y = _forward_y(engine, row_ptr, Q, K, V, heads, sc, bf16, y64)
        want = abr.attention_bwd_ref(row_ptr, ids, Q, K, V, G, y, n, d, dv, heads, sc, *bf16)
        for short in (256, 0):
            engine.set_option("attn_short", short)
            got, st = _call(engine, row_ptr, Q, K, V, G, y, heads, scale, bf16)
            _same(got, want, (bf16, scale, short))
            ref = abr.attention_bwd_stats_ref(row_ptr, ids, n, short)
            assert {k: st[k] for k in ref} == ref
    engine.set_option("attn_short", 256)


def test_real_held_results_equal_the_twin(engine, tiny_dangling):
    """the held result of a query, of a top-64 query and of a seed-set call work as the injected rows do"""
    g = tiny_dangling
    srcs = _mixed_sources(g, 9970)                # a duplicate and a dangling source
    _load(engine, g)
    row_ptr, ids, vals, st, sp = engine.query_sparse(srcs, threshold=0.0)
    _check_held(engine, row_ptr, ids, g.n, 9970)
    row_ptr, ids, vals, st, sp, tk = engine.query_sparse_topk(srcs, 64, threshold=0.0)
    assert int(np.diff(row_ptr).max()) == 64
    _check_held(engine, row_ptr, ids, g.n, 9980)
    live = [int(s) for s in srcs if g.deg[s] > 0]
    r = engine.query_seeds_sparse([live[:3], live[2:5]], [[0.5, 0.25, 0.25], [3.0, 1.0, 2.0]], threshold=1.0 / g.n)
    _check_held(engine, r["row_ptr"], r["ids"], g.n, 9990)


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def _raw(engine, row_ptr, nq, q, k, v, g, y, ycap, d, dv, heads, scale, outs, lds, types=(0, 0, 0, 0, 0), ld=None, grads=True):
    """the C call itself.  outs: (dq32, dq64, dk32, dk64, dv32, dv64) numpy arrays or None; lds: (lddq, lddk, lddv)"""
    ldq, ldk, ldv, ldg = ld or tuple(x.strides[0] // x.itemsize if x is not None else 1 for x in (q, k, v, g))
    gr = capi.AttnGrads()
    for name, a32, a64, l in zip(("dq", "dk", "dv"), outs[0::2], outs[1::2], lds):
        setattr(gr, name + "32", _p(a32).value if a32 is not None else None)
        setattr(gr, name + "64", _p(a64).value if a64 is not None else None)
        setattr(gr, "ld" + name, l)
    return engine._lib.fora_hip_sparse_attention_bwd(engine._ctx, _p(row_ptr), C.c_int(nq), _p(q), C.c_int(int(types[0])), C.c_int64(ldq), _p(k), C.c_int(int(types[1])),
                                                     C.c_int64(ldk), _p(v), C.c_int(int(types[2])), C.c_int64(ldv), _p(g), C.c_int(int(types[3])), C.c_int64(ldg),
                                                     _p(y), C.c_int(int(types[4])), C.c_uint64(ycap), C.c_int(d), C.c_int(dv), C.c_int(heads), C.c_double(scale),
                                                     C.byref(gr) if grads else None, None)


def test_argument_errors(engine, tiny):
    g = tiny
    _load(engine, g)
    srcs = _mixed_sources(g, 9995)
    nq, d, dv, heads = len(srcs), 4, 3, 2
    engine.sparse_clear()
    Q, K, V, G = (np.ascontiguousarray(x) for x in _operands(nq, g.n, d, dv, heads, (False,) * 4, seed=9995))
    big = 1 << 20
    y = np.full(big, 0.25, np.float32)
    w, wv = heads * d, heads * dv
    outs = [np.full((nq, w), -5.0, np.float32), np.full((nq, w), -5.0, np.float64), np.full((g.n, w), -5.0, np.float32), np.full((g.n, w), -5.0, np.float64),
            np.full((g.n, wv), -5.0, np.float32), np.full((g.n, wv), -5.0, np.float64)]
    call = lambda rp=None, n_=nq, q=Q, k=K, v=V, g_=G, y_=y, cap=big, d_=d, dv_=dv, h=heads, sc=0.5, o=outs, lds=(w, w, wv), types=(0, 0, 0, 0, 0), \
        ld=(w, w, wv, wv), grads=True: _raw(engine, rp, n_, q, k, v, g_, y_, cap, d_, dv_, h, sc, o, lds, types=types, ld=ld, grads=grads)
    assert call(np.zeros(nq + 1, np.int64)) == -1                                       # no held result
    row_ptr, ids, vals, st, sp = engine.query_sparse(srcs, threshold=1.0 / g.n)
    e = sp["entries"]
    assert 0 < heads * e <= big
    gen = engine.get_option("sparse_generation")
    end, dec, first, short = row_ptr.copy(), row_ptr.copy(), row_ptr.copy(), row_ptr.copy()
    end[-1] += 1
    dec[2] = dec[1] - 1
    first[0] = 1
    short[-1] -= 1
    for bad in (end, short, dec, first, None):
        assert call(bad) == -1                                                          # a row_ptr that is not the held result's
    ok = lambda **kw: call(row_ptr, **kw)
    assert ok(n_=-1) == -1
    assert ok(q=None) == -1 and ok(k=None) == -1 and ok(v=None) == -1 and ok(g_=None) == -1 and ok(y_=None) == -1      # a NULL operand with entries to read
    for t in ((2, 0, 0, 0, 0), (0, 3, 0, 0, 0), (0, 0, 2, 0, 0), (0, 0, 0, 2, 0), (-1, 0, 0, 0, 0), (0, 0, 0, 0, 1), (0, 0, 0, 0, 3), (0, 0, 0, 0, -1)):
        assert ok(types=t) == -1                                                        # f64 is no operand type, bf16 is no y type
    assert ok(d_=0) == -1 and ok(dv_=0) == -1 and ok(d_=65537, h=1) == -1 and ok(dv_=65537, h=1) == -1
    assert ok(h=0) == -1 and ok(h=-2) == -1
    huge = (1 << 20,) * 4
    assert ok(d_=1, h=65537, ld=huge, lds=huge[:3]) == -1                               # heads * d over 65536
    assert ok(d_=40000, dv_=1, h=2, ld=huge, lds=huge[:3]) == -1
    assert ok(d_=1, dv_=40000, h=2, ld=huge, lds=huge[:3]) == -1
    for i in range(4):
        assert ok(ld=tuple(x - (k == i) for k, x in enumerate((w, w, wv, wv)))) == -1    # a pitch smaller than the width
    for i in range(3):
        assert ok(lds=tuple(x - (k == i) for k, x in enumerate((w, w, wv)))) == -1
    for bad_scale in (np.nan, np.inf, -np.inf):
        assert ok(sc=bad_scale) == -1
    assert ok(o=[None] * 6) == -1 and ok(grads=False) == -1                             # all three gradients absent
    assert ok(cap=heads * e - 1) == -1                                                  # ycap too small
    assert all((o == -5.0).all() for o in outs)                                         # nothing was written
    i2 = np.zeros(e, np.int32)
    assert _raw_fetch(engine, i2, None, None, e) == 0 and (i2 == ids).all() and engine.get_option("sparse_generation") == gen      # the held result is intact
    # ... and usable: an absent gradient's pitch is not read; ycap may be exactly heads * entries
    yv = np.ascontiguousarray(_forward_y(engine, row_ptr, Q, K, V, heads, 0.5, (False,) * 3, False).reshape(-1))
    assert call(row_ptr, y_=yv, cap=heads * e, o=outs[:2] + [None] * 4, lds=(w, 0, 0)) == 0
    want = abr.attention_bwd_ref(row_ptr, ids, Q, K, V, G, yv.reshape(heads, e), g.n, d, dv, heads, 0.5)
    assert (_b64(outs[1]) == _b64(want[0])).all() and (_b32(outs[0]) == _b32(want[0].astype(np.float32))).all()
    assert all((o == -5.0).all() for o in outs[2:])
    assert call(row_ptr, y_=yv, cap=heads * e) == 0
    assert (_b64(outs[3]) == _b64(want[1])).all() and (_b64(outs[5]) == _b64(want[2])).all()
    assert engine.get_option("sparse_generation") == gen
    # the binding refuses what the C ABI cannot express
    y2 = yv.reshape(heads, e)
    with pytest.raises(ValueError):
        engine.sparse_attention_bwd(row_ptr, Q, K, V, G, y2, heads=3)
    with pytest.raises(ValueError):
        engine.sparse_attention_bwd(row_ptr, Q, K, V, G[:, :-1], y2, heads=heads)
    with pytest.raises(ValueError):
        engine.sparse_attention_bwd(row_ptr, Q, K, V, G, y2[:1], heads=heads)
    with pytest.raises(ValueError):
        engine.sparse_attention_bwd(row_ptr, Q, K, V, G, y2.astype(np.float16), heads=heads)
    # nq == 0, an empty held result: FORA_OK, nothing written
    engine.query_sparse(np.zeros(0, np.int32))
    for o in outs:
        o[:] = -5.0
    assert call(np.zeros(1, np.int64), n_=0, q=None, k=None, v=None, g_=None, y_=None, cap=0) == 0
    assert all((o == -5.0).all() for o in outs)


def test_device_operands_and_outputs():
    """Q, K, V, G, y and the outputs as torch tensors on the GPU, in a fresh child process (tests/attention_bwd_device_child.py):
    torch and the library must live on one HIP runtime, so the child imports torch before the library is loaded."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "attention_bwd_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "attention bwd device ok" in r.stdout
