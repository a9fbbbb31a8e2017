"""ATTENTION (fora_hip_sparse_attention) on the GPU: scores, softmax and the weighted product over the held rows in one call, bit
for bit against the numpy twin of the contract (tests/attention_ref.py) and against the three existing calls chained through
float64 on the same engine.  Every equality is on the bits of out64 and y64; out32 and y32 are checked as (float) of them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import attention_ref as ar
import softmax_ref as sm
from test_sparse_gpu import SEED, _mixed_sources, _raw_fetch

pytestmark = pytest.mark.gpu
ROW_LENS, EMPTY = sm.ROW_LENS, sm.EMPTY
QNAN = 0x7FF8000000000000

# (d, dv, heads, (q, k, v) as bf16, scale, (pitch padding, first column) of the wider arrays the operands are slices of).  d covers
# every lane-group width of the scores (1, 4, 32, 64) and a second column per lane (65, 200); dv a lane's single column, a partial
# tile, a full wave, a tail lane behind vector loads (130); the paddings make the pitches of case 2 and 6 odd (one column per
# load) and keep those of cases 3, 4, 5 and 7 multiples of the widest vector.
CASES = [
    (1, 1, 3, (False, False, False), 1.0, (0, 0)),
    (3, 5, 2, (True, False, True), 0.37, (3, 1)),
    (32, 64, 1, (False, True, False), -2.0, (4, 0)),
    (64, 130, 1, (True, True, True), 0.0, (6, 0)),
    (65, 64, 2, (False, False, False), 0.37, (0, 0)),
    (200, 5, 1, (False, False, True), 1.0, (1, 1)),
    (64, 64, 3, (False, True, True), -2.0, (8, 0)),
    (3, 130, 2, (True, False, False), 0.37, (2, 0)),
]


def _load(engine, g, **kw):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(seed=SEED, epsilon=0.5, **kw)


def _slice(X, pad, off, bf16):
    """X as columns [off, off + w) of an array of w + pad + off columns whose other columns hold NaN patterns never to be read"""
    w = X.shape[1]
    return ar.padded(np.concatenate([np.zeros((X.shape[0], off), np.float32), X], axis=1), w + pad + off, bf16)[:, off:off + w]


def _operands(nq, n, d, dv, heads, bf16, pad=(0, 0), seed=9800):
    rng = np.random.Generator(np.random.PCG64(seed + 7 * d + dv))
    Q, K = ar.scores_operands(rng, nq, n, d, heads)
    V = (rng.standard_normal((n, heads * dv)) * np.exp2(rng.integers(-6, 7, size=(n, heads * dv)))).astype(np.float32)
    return tuple(_slice(X, pad[0], pad[1], b) for X, b in zip((Q, K, V), bf16))


@pytest.fixture(scope="module")
def held(engine_test, tiny):
    """the held result of the injected rows on the test build's engine, and the twins of the cases -- made once, never changed"""
    _load(engine_test, tiny)
    rows_fix = sm.injected_rows(tiny.n)
    h = {"n": tiny.n, "nq": len(ROW_LENS), "twin": {}}

    def hold():
        row_ptr, sp = engine_test.test_sparse_rows(rows_fix, threshold=0.0)
        assert (np.diff(row_ptr) == ROW_LENS).all()
        e = int(row_ptr[-1])
        ids = np.zeros(e, np.int32)
        assert _raw_fetch(engine_test, ids, None, None, e) == 0
        h.update(row_ptr=row_ptr, ids=ids, entries=e)
    h["hold"] = hold
    hold()
    return h


def _reset(engine):
    engine.set_batch(0)
    for k, v in (("prop_segs", 0), ("softmax_short", 256), ("attn_short", 256)):
        engine.set_option(k, v)


def _ensure_held(engine_test, tiny, held):
    """another module may have used the session's test engine in between: put graph and rows back if so"""
    e = held["entries"]
    ids = np.zeros(e, np.int32)
    if engine_test.n != tiny.n or _raw_fetch(engine_test, ids, None, None, e) != 0 or not (ids == held["ids"]).all():
        _load(engine_test, tiny)
        held["hold"]()
    _reset(engine_test)


def _twin(held, case):
    if case not in held["twin"]:
        d, dv, heads, bf16, scale, pad = CASES[case]
        Q, K, V = _operands(held["nq"], held["n"], d, dv, heads, bf16, pad)
        held["twin"][case] = (Q, K, V, ar.attention_ref(held["row_ptr"], held["ids"], Q, K, V, d, dv, heads, scale, *bf16))
    return held["twin"][case]


def _same(got, want, what):
    """(out32, out64, y32, y64) of the engine against (out64, out32, y64, y32) of the twin"""
    o32, o64, y32, y64 = got
    w64, w32, wy64, wy32 = want[:4]
    assert (o64.view(np.uint64) == w64.view(np.uint64)).all(), what
    assert (y64.view(np.uint64) == wy64.view(np.uint64)).all(), what
    assert (o32.view(np.uint32) == w32.view(np.uint32)).all() and (y32.view(np.uint32) == wy32.view(np.uint32)).all(), what
    with np.errstate(over="ignore"):
        assert (o32.view(np.uint32) == o64.astype(np.float32).view(np.uint32)).all() and (y32.view(np.uint32) == y64.astype(np.float32).view(np.uint32)).all(), what


def _call(engine, row_ptr, Q, K, V, heads, scale, bf16, **kw):
    r = engine.sparse_attention(row_ptr, Q, K, V, heads=heads, scale=scale, want64=True, want_y32=True, want_y64=True,
                                q_bf16=bf16[0], k_bf16=bf16[1], v_bf16=bf16[2], **kw)
    return r[:4], r[4]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_equals_the_twin_on_both_paths(engine_test, tiny, held, case):
    _ensure_held(engine_test, tiny, held)
    d, dv, heads, bf16, scale, pad = CASES[case]
    Q, K, V, want = _twin(held, case)
    assert want[4] == 0 and np.isfinite(want[0]).all()
    if scale:                                            # the scores are spread: the largest y of the longest row is well above the smallest
        y = want[2][0, held["row_ptr"][-3]:held["row_ptr"][-2]]
        assert y.max() / max(y.min(), 1e-300) > 1e6 or d == 1
    for short in (256, 0):
        engine_test.set_option("attn_short", short)
        got, st = _call(engine_test, held["row_ptr"], Q, K, V, heads, scale, bf16)
        assert got[1].shape == (held["nq"], heads * dv) and got[3].shape == (heads, held["entries"])
        _same(got, want, (CASES[case], short))
        ref = ar.attention_stats_ref(held["row_ptr"], short)
        assert {k: st[k] for k in ref} == ref and st["nan_rows"] == 0 and st["attn_ms"] >= 0.0
        assert st["q_on_device"] == st["k_on_device"] == st["v_on_device"] == 0
        assert (got[1][EMPTY].view(np.uint64) == 0).all()                     # the empty row: +0.0
    engine_test.set_option("attn_short", 256)


@pytest.mark.parametrize("case", [1, 4, 6])
def test_equals_the_three_calls_chained_through_f64(engine_test, tiny, held, case):
    _ensure_held(engine_test, tiny, held)
    d, dv, heads, bf16, scale, pad = CASES[case]
    Q, K, V, _ = _twin(held, case)
    row_ptr = held["row_ptr"]
    for short in (256, 0):
        engine_test.set_option("attn_short", short)
        (o32, o64, y32, y64), _ = _call(engine_test, row_ptr, Q, K, V, heads, scale, bf16)
        for j in range(heads):
            qs, vs = slice(j * d, (j + 1) * d), slice(j * dv, (j + 1) * dv)
            _, s64, _ = engine_test.sparse_sddmm(row_ptr, Q[:, qs], K[:, qs], want32=False, want64=True, a_bf16=bf16[0], b_bf16=bf16[1])
            _, p64, _ = engine_test.sparse_softmax(row_ptr, s64, scale=scale, want32=False, want64=True)
            _, c64, _ = engine_test.sparse_propagate(row_ptr, V[:, vs], want32=False, want64=True, bf16=bf16[2], values=p64)
            assert (y64[j].view(np.uint64) == p64.view(np.uint64)).all(), (case, short, j)
            assert (o64[:, vs].view(np.uint64) == c64.view(np.uint64)).all(), (case, short, j)
    engine_test.set_option("attn_short", 256)


def test_options_and_batch_change_no_bit(engine_test, tiny, held):
    _ensure_held(engine_test, tiny, held)
    case = 1
    d, dv, heads, bf16, scale, pad = CASES[case]
    Q, K, V, want = _twin(held, case)
    try:
        for short, b, segs, sshort in ((0, 0, 0, 256), (1, 1, 1, 0), (64, 7, 3, 64), (256, 0, 2, 1), (1000, 3, 0, 256), (0, 2, 1, 0)):
            engine_test.set_option("attn_short", short)
            engine_test.set_batch(b)
            engine_test.set_option("prop_segs", segs)
            engine_test.set_option("softmax_short", sshort)
            got, st = _call(engine_test, held["row_ptr"], Q, K, V, heads, scale, bf16)
            _same(got, want, (short, b, segs, sshort))
            ref = ar.attention_stats_ref(held["row_ptr"], short)
            assert {k: st[k] for k in ref} == ref, (short, st)
        assert ar.attention_stats_ref(held["row_ptr"], 64)["short_rows"] == 5 and ar.attention_stats_ref(held["row_ptr"], 0)["long_rows"] == 10
    finally:
        _reset(engine_test)


def test_nan_rows_on_both_paths(engine_test, tiny, held):
    """a NaN and a +inf in rows of K whose ids lie in a short and in a long row: those (row, head) pairs are the quiet NaN in out
    and y and are counted, every other one keeps its bits"""
    _ensure_held(engine_test, tiny, held)
    d, dv, heads, bf16, scale = 5, 6, 2, (False, False, False), 0.37
    row_ptr, ids = held["row_ptr"], held["ids"]
    row = {L: i for i, L in enumerate(ROW_LENS)}
    Q, K, V = _operands(held["nq"], held["n"], d, dv, heads, bf16, seed=9810)
    clean = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, scale)
    K = K.copy()
    id_nan, id_inf = int(ids[row_ptr[row[63]] + 40]), int(ids[row_ptr[row[600]] + 599])
    c_inf = d + int(np.argmax(Q[row[600], d:2 * d]))      # a column of head 1 where the long row's q is positive: its score is +inf
    assert Q[row[600], c_inf] > 0
    K[id_nan, 2] = np.nan                                # head 0
    K[id_inf, c_inf] = np.inf                            # head 1
    want = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, scale)
    # a row that keeps id_nan is a NaN row of head 0; one that keeps id_inf is one of head 1 unless its q there is negative: then the
    # score is -inf, the entry's y is +0.0 and the row is an ordinary one
    hit = {(i, 0) for i in range(held["nq"]) if id_nan in ids[row_ptr[i]:row_ptr[i + 1]]}
    hit |= {(i, 1) for i in range(held["nq"]) if id_inf in ids[row_ptr[i]:row_ptr[i + 1]] and not Q[i, c_inf] < 0}
    assert (row[63], 0) in hit and (row[600], 1) in hit and want[4] == len(hit)
    for short in (256, 0, 64):
        engine_test.set_option("attn_short", short)
        got, st = _call(engine_test, row_ptr, Q, K, V, heads, scale, bf16)
        _same(got, want, short)
        assert st["nan_rows"] == len(hit)
        o32, o64, y32, y64 = got
        for i in range(held["nq"]):
            for j in range(heads):
                o, y = o64[i, j * dv:(j + 1) * dv], y64[j, row_ptr[i]:row_ptr[i + 1]]
                if (i, j) in hit:
                    assert (o.view(np.uint64) == QNAN).all() and (y.view(np.uint64) == QNAN).all()
                    assert (o32[i, j * dv:(j + 1) * dv].view(np.uint32) == 0x7FC00000).all() and (y32[j, row_ptr[i]:row_ptr[i + 1]].view(np.uint32) == 0x7FC00000).all()
                elif (id_nan, id_inf)[j] not in ids[row_ptr[i]:row_ptr[i + 1]]:      # (untouched by the change of K)
                    assert (o.view(np.uint64) == clean[0][i, j * dv:(j + 1) * dv].view(np.uint64)).all()
                    assert (y.view(np.uint64) == clean[2][j, row_ptr[i]:row_ptr[i + 1]].view(np.uint64)).all()
                else:
                    assert np.isfinite(o).all() and (y[ids[row_ptr[i]:row_ptr[i + 1]] == id_inf].view(np.uint64) == 0).all()      # -inf: +0.0
        # the chained calls agree in NaN-ness on those rows and in bits on the others
        for j in range(heads):
            _, s64, _ = engine_test.sparse_sddmm(row_ptr, Q[:, j * d:(j + 1) * d], K[:, j * d:(j + 1) * d], want32=False, want64=True)
            _, p64, _ = engine_test.sparse_softmax(row_ptr, s64, scale=scale, want32=False, want64=True)
            _, c64, _ = engine_test.sparse_propagate(row_ptr, V[:, j * dv:(j + 1) * dv], want32=False, want64=True, values=p64)
            mine = o64[:, j * dv:(j + 1) * dv]
            assert (np.isnan(c64) == np.isnan(mine)).all() and (c64[~np.isnan(c64)].view(np.uint64) == mine[~np.isnan(mine)].view(np.uint64)).all()
    engine_test.set_option("attn_short", 256)


def test_partial_outputs_and_tails(engine_test, tiny, held):
    _ensure_held(engine_test, tiny, held)
    case = 1
    d, dv, heads, bf16, scale, pad = CASES[case]
    Q, K, V, want = _twin(held, case)
    row_ptr, e, nq = held["row_ptr"], held["entries"], held["nq"]
    kw = dict(heads=heads, scale=scale, q_bf16=bf16[0], k_bf16=bf16[1], v_bf16=bf16[2])
    for short in (256, 0):
        engine_test.set_option("attn_short", short)
        a32, a64, ay32, ay64, _ = engine_test.sparse_attention(row_ptr, Q, K, V, **kw)
        assert a64 is None and ay32 is None and ay64 is None and (a32.view(np.uint32) == want[1].view(np.uint32)).all()
        b32, b64, by32, by64, _ = engine_test.sparse_attention(row_ptr, Q, K, V, want32=False, want64=True, want_y64=True, **kw)
        assert b32 is None and by32 is None and (b64.view(np.uint64) == want[0].view(np.uint64)).all() and (by64.view(np.uint64) == want[2].view(np.uint64)).all()
        _, _, cy32, cy64, _ = engine_test.sparse_attention(row_ptr, Q, K, V, want_y32=True, **kw)
        assert cy64 is None and (cy32.view(np.uint32) == want[3].view(np.uint32)).all()
        # caller-made outputs wider than heads * dv keep their other columns; y arrays longer than heads * entries keep their tail
        w32, w64 = np.full((nq, heads * dv + 3), -7.0, np.float32), np.full((nq, heads * dv + 3), -7.0, np.float64)
        engine_test.sparse_attention(row_ptr, Q, K, V, out32=w32[:, :heads * dv], out64=w64[:, :heads * dv], **kw)
        assert (w64[:, :heads * dv].view(np.uint64) == want[0].view(np.uint64)).all() and (w32[:, :heads * dv].view(np.uint32) == want[1].view(np.uint32)).all()
        assert (w32[:, heads * dv:] == -7.0).all() and (w64[:, heads * dv:] == -7.0).all()
        ly32, ly64 = np.full(heads * e + 5, -7.0, np.float32), np.full(heads * e + 5, -7.0, np.float64)
        o32 = np.zeros((nq, heads * dv), np.float32)
        assert _raw(engine_test, row_ptr, nq, Q, K, V, d, dv, heads, scale, o32, None, heads * dv, ly32, ly64, heads * e + 5, types=bf16) == 0
        assert (ly64[:heads * e].view(np.uint64) == want[2].reshape(-1).view(np.uint64)).all() and (ly32[:heads * e].view(np.uint32) == want[3].reshape(-1).view(np.uint32)).all()
        assert (ly32[heads * e:] == -7.0).all() and (ly64[heads * e:] == -7.0).all() and (o32.view(np.uint32) == want[1].view(np.uint32)).all()
    engine_test.set_option("attn_short", 256)


def _check_held(engine, row_ptr, ids, n, seed):
    d, dv, heads = 8, 6, 2
    nq = len(row_ptr) - 1
    for bf16, scale in (((False, False, False), None), ((True, True, True), -2.0)):
        Q, K, V = _operands(nq, n, d, dv, heads, bf16, seed=seed)
        sc = float(d) ** -0.5 if scale is None else scale
        want = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, sc, *bf16)
        for short in (256, 0):
            engine.set_option("attn_short", short)
            got, st = _call(engine, row_ptr, Q, K, V, heads, scale, bf16)
            _same(got, want, (bf16, scale, short))
            ref = ar.attention_stats_ref(row_ptr, short)
            assert {k: st[k] for k in ref} == ref and st["nan_rows"] == want[4] == 0
    engine.set_option("attn_short", 256)


def test_real_held_results_equal_the_twin(engine, tiny_dangling):
    """the held result of a query, of a top-64 query and of a seed-set call work as the injected rows do"""
    g = tiny_dangling
    srcs = _mixed_sources(g, 9820)                # a duplicate and a dangling source
    _load(engine, g)
    row_ptr, ids, vals, st, sp = engine.query_sparse(srcs, threshold=0.0)
    _check_held(engine, row_ptr, ids, g.n, 9820)
    row_ptr, ids, vals, st, sp, tk = engine.query_sparse_topk(srcs, 64, threshold=0.0)
    assert int(np.diff(row_ptr).max()) == 64
    _check_held(engine, row_ptr, ids, g.n, 9830)
    live = [int(s) for s in srcs if g.deg[s] > 0]
    r = engine.query_seeds_sparse([live[:3], live[2:5]], [[0.5, 0.25, 0.25], [3.0, 1.0, 2.0]], threshold=1.0 / g.n)
    _check_held(engine, r["row_ptr"], r["ids"], g.n, 9840)


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def _raw(engine, row_ptr, nq, q, k, v, d, dv, heads, scale, o32, o64, ldo, y32, y64, ycap, types=(0, 0, 0), ld=None):
    ldq, ldk, ldv = ld or tuple(x.strides[0] // x.itemsize if x is not None else 1 for x in (q, k, v))
    return engine._lib.fora_hip_sparse_attention(engine._ctx, _p(row_ptr), C.c_int(nq), _p(q), C.c_int(int(types[0])), C.c_int64(ldq), _p(k), C.c_int(int(types[1])),
                                                 C.c_int64(ldk), _p(v), C.c_int(int(types[2])), C.c_int64(ldv), C.c_int(d), C.c_int(dv), C.c_int(heads),
                                                 C.c_double(scale), _p(o32), _p(o64), C.c_int64(ldo), _p(y32), _p(y64), C.c_uint64(ycap), None)


def test_argument_errors(engine, tiny):
    g = tiny
    _load(engine, g)
    srcs = _mixed_sources(g, 9850)
    nq, d, dv, heads = len(srcs), 4, 3, 2
    engine.sparse_clear()
    Q, K, V = _operands(nq, g.n, d, dv, heads, (False, False, False), seed=9850)
    Q, K, V = (np.ascontiguousarray(x) for x in (Q, K, V))
    big = 1 << 20
    o32, o64 = np.full((nq, heads * dv), -5.0, np.float32), np.full((nq, heads * dv), -5.0, np.float64)
    y32, y64 = np.full(big, -5.0, np.float32), np.full(big, -5.0, np.float64)
    w = heads * d
    call = lambda rp=None, n_=nq, q=Q, k=K, v=V, d_=d, dv_=dv, h=heads, sc=0.5, a=o32, b=o64, ldo=heads * dv, c=y32, e_=y64, cap=big, types=(0, 0, 0), \
        ld=(w, w, heads * dv): _raw(engine, rp, n_, q, k, v, d_, dv_, h, sc, a, b, ldo, c, e_, cap, types=types, ld=ld)
    assert call(np.zeros(nq + 1, np.int64)) == -1                                       # no held result
    row_ptr, ids, vals, st, sp = engine.query_sparse(srcs, threshold=1.0 / g.n)
    e = sp["entries"]
    assert 0 < heads * e <= big
    end, dec, first, short = row_ptr.copy(), row_ptr.copy(), row_ptr.copy(), row_ptr.copy()
    end[-1] += 1
    dec[2] = dec[1] - 1
    first[0] = 1
    short[-1] -= 1
    for bad in (end, short, dec, first, None):
        assert call(bad) == -1                                                          # a row_ptr that is not the held result's
    ok = lambda **kw: call(row_ptr, **kw)
    assert ok(n_=-1) == -1
    assert ok(q=None) == -1 and ok(k=None) == -1 and ok(v=None) == -1                   # a NULL operand with entries to read
    for t in ((2, 0, 0), (0, 3, 0), (0, 0, 2), (-1, 0, 0)):
        assert ok(types=t) == -1                                                        # f64 or anything else is no operand type
    assert ok(d_=0) == -1 and ok(dv_=0) == -1 and ok(d_=65537, h=1) == -1 and ok(dv_=65537, h=1) == -1
    assert ok(h=0) == -1 and ok(h=-2) == -1
    assert ok(d_=1, h=65537, ld=(1 << 20, 1 << 20, 1 << 20), ldo=1 << 20) == -1         # heads * d over 65536
    assert ok(d_=40000, dv_=1, h=2, ld=(1 << 20, 1 << 20, 1 << 20)) == -1
    assert ok(d_=1, dv_=40000, h=2, ld=(1 << 20, 1 << 20, 1 << 20), ldo=1 << 20) == -1
    assert ok(ld=(w - 1, w, heads * dv)) == -1 and ok(ld=(w, w - 1, heads * dv)) == -1 and ok(ld=(w, w, heads * dv - 1)) == -1
    assert ok(ldo=heads * dv - 1) == -1                                                 # a pitch smaller than the width
    for bad_scale in (np.nan, np.inf, -np.inf):
        assert ok(sc=bad_scale) == -1
    assert ok(a=None, b=None) == -1                                                     # both outs NULL
    assert ok(cap=heads * e - 1) == -1 and ok(c=None, cap=heads * e - 1) == -1 and ok(e_=None, cap=0) == -1      # ycap too small for a y output
    assert (o32 == -5.0).all() and (o64 == -5.0).all() and (y32 == -5.0).all() and (y64 == -5.0).all()        # nothing was written
    i2 = np.zeros(e, np.int32)
    assert _raw_fetch(engine, i2, None, None, e) == 0 and (i2 == ids).all()              # the held result is intact
    assert ok(c=None, e_=None, cap=0) == 0                                              # ... and usable; no y output needs no ycap
    want = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, 0.5)
    assert (o64.view(np.uint64) == want[0].view(np.uint64)).all() and (o32.view(np.uint32) == want[1].view(np.uint32)).all()
    assert (y32 == -5.0).all() and (y64 == -5.0).all()
    # the binding refuses what the C ABI cannot express
    with pytest.raises(ValueError):
        engine.sparse_attention(row_ptr, Q, K, V, heads=3)
    with pytest.raises(ValueError):
        engine.sparse_attention(row_ptr, Q, K[:, :-1], V, heads=1)
    with pytest.raises(ValueError):
        engine.sparse_attention(row_ptr, Q.astype(np.float64), K, V, heads=heads)
    # nq == 0, an empty held result: FORA_OK, nothing written
    engine.query_sparse(np.zeros(0, np.int32))
    o32[:] = -5.0
    assert call(np.zeros(1, np.int64), n_=0, q=None, k=None, v=None, b=None, c=None, e_=None, cap=0, ld=(w, w, heads * dv)) == 0
    assert (o32 == -5.0).all()


def test_device_operands_and_outputs():
    """Q, K, V and the outputs as torch tensors on the GPU, in a fresh child process (tests/attention_device_child.py): torch and
    the library must live on one HIP runtime, so the child imports torch before the library is loaded."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "attention_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "attention device ok" in r.stdout
