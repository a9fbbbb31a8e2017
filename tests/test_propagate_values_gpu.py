"""PROPAGATE WITH VALUES (fora_hip_sparse_propagate_vals, fora_hip_sparse_propagate_t_vals) on the GPU: the two products with
the caller's values on the held pattern, bit for bit against the numpy twin (tests/propagate_values_ref.py).  The values are
all different and scaled over 2^+-20, so a value read from the wrong place -- a wrong pos in the transposed product --
changes bits.  Every bit-order assertion is made on out64; out32 is checked as (float)out64."""
import ctypes as C

import numpy as np
import pytest

import propagate_ref as pr
import propagate_t_ref as pt
import propagate_values_ref as pv
import sddmm_ref as sr
from test_sparse_gpu import SEED, _raw_fetch

pytestmark = pytest.mark.gpu
CAPS = (0, 64, pt.LDS_MAX)                     # "propt_lds_cap": every run global, medium runs global, the default
EMPTY_ROW = 300                                # of propagate_t_ref.injected_columns


def _load(engine, g, **kw):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(seed=SEED, epsilon=0.5, **kw)


@pytest.fixture(scope="module")
def injected(engine_test, tiny):
    """the held result of the injected columns on the test build's engine, its fetched arrays, one set of values of each
    type -- made once, never changed"""
    _load(engine_test, tiny)
    rows_fix, col_lens = pt.injected_columns(tiny.n)
    want_ptr, want_ids, want_fix = pt.csr_of(rows_fix)
    held = {"n": tiny.n, "nq": rows_fix.shape[0], "col_lens": col_lens, "twins": {}}

    def hold():
        row_ptr, sp = engine_test.test_sparse_rows(rows_fix, threshold=0.0)
        assert (row_ptr == want_ptr).all()
        e = int(row_ptr[-1])
        ids, fix, vals = np.zeros(e, np.int32), np.zeros(e, np.uint64), np.zeros(e, np.float64)
        assert _raw_fetch(engine_test, ids, vals, fix, e) == 0
        assert (ids == want_ids).all() and (fix == want_fix).all()
        held.update(row_ptr=row_ptr, ids=ids, fix=fix, vals=vals, entries=e)
    held["hold"] = hold
    hold()
    rng = np.random.Generator(np.random.PCG64(9200))
    held["col_ptr"] = pt.transpose_ref(held["row_ptr"], held["ids"], held["fix"], tiny.n)[0]
    held["values"] = {np.float32: pv.distinct_values(rng, held["entries"], np.float32), np.float64: pv.distinct_values(rng, held["entries"], np.float64)}
    return held


def _ensure_held(engine_test, tiny, injected):
    """another module may have used the session's test engine in between: put graph and rows back if so"""
    e = injected["entries"]
    ids = np.zeros(e, np.int32)
    if engine_test.n != tiny.n or _raw_fetch(engine_test, ids, None, None, e) != 0 or not (ids == injected["ids"]).all():
        _load(engine_test, tiny)
        injected["hold"]()
    engine_test.set_option("propt_lds_cap", pt.LDS_MAX)
    engine_test.set_option("prop_segs", 0)


_dense = sr.operand      # [rows, d] as a view of a [rows, ld] array with NaN padding


def _twin_fwd(injected, d, bf16, vt):
    key = ("fwd", d, bf16, vt)
    if key not in injected["twins"]:
        H = _dense(injected["n"], d, d, bf16, 9300 + d)
        injected["twins"][key] = pv.propagate_vals_ref(injected["row_ptr"], injected["ids"], injected["values"][vt], H, bf16=bf16)
    return injected["twins"][key]


def _twin_t(injected, d, bf16, vt):
    key = ("t", d, bf16, vt)
    if key not in injected["twins"]:
        G = _dense(injected["nq"], d, d, bf16, 9400 + d, nan_row=EMPTY_ROW)
        injected["twins"][key] = pv.propagate_t_vals_ref(injected["row_ptr"], injected["ids"], injected["values"][vt], G, injected["n"], bf16=bf16)
    return injected["twins"][key]


def _same(got64, got32, want64, want32, what):
    assert (got64.view(np.uint64) == want64.view(np.uint64)).all(), what
    assert (got32.view(np.uint32) == want32.view(np.uint32)).all(), what
    assert (got32.view(np.uint32) == got64.astype(np.float32).view(np.uint32)).all(), what


@pytest.mark.parametrize("d", [1, 3, 16, 65])
def test_both_products_equal_the_twin(engine_test, tiny, injected, d):
    _ensure_held(engine_test, tiny, injected)
    n, nq, row_ptr = injected["n"], injected["nq"], injected["row_ptr"]
    try:
        for bf16 in (False, True):
            elt = 2 if bf16 else 4
            for vt in (np.float32, np.float64):
                values = injected["values"][vt]
                # ---- forward: out = P(values) x H, at two pitches
                want64, want32 = _twin_fwd(injected, d, bf16, vt)
                for ldf in (d, d + 3):
                    H = _dense(n, d, ldf, bf16, 9300 + d)
                    o32, o64, ps = engine_test.sparse_propagate(row_ptr, H, bf16=bf16, want64=True, values=values)
                    _same(o64, o32, want64, want32, ("fwd", d, bf16, vt, ldf))
                    ref = pr.prop_stats_ref(row_ptr, d, elt)
                    assert {k: ps[k] for k in ref} == ref
                assert not np.signbit(o64[EMPTY_ROW]).any() and (o64[EMPTY_ROW] == 0.0).all()       # an empty row: +0.0
                # ---- transposed: out = P(values)^T x G, on every sort tier
                want64, want32 = _twin_t(injected, d, bf16, vt)
                assert np.isfinite(want64).all()                                                      # row 300 of G, all NaN, reaches no output
                for cap in CAPS:
                    engine_test.set_option("propt_lds_cap", cap)                                      # a change drops the transposition, and pos with it
                    G = _dense(nq, d, d + (cap == 64), bf16, 9400 + d, nan_row=EMPTY_ROW)
                    o32, o64, ps = engine_test.sparse_propagate_t(row_ptr, G, bf16=bf16, want64=True, values=values)
                    _same(o64, o32, want64, want32, ("t", d, bf16, vt, cap))
                    tiers = pt.tier_counts(injected["col_ptr"], cap)                                  # (every cap differs from the one before it)
                    assert ps["built"] == 1 and {k: ps[k] for k in tiers} == tiers, (cap, ps)
    finally:
        engine_test.set_option("propt_lds_cap", pt.LDS_MAX)


def test_prop_segs_changes_no_bit(engine_test, tiny, injected):
    _ensure_held(engine_test, tiny, injected)
    n, nq, row_ptr, d = injected["n"], injected["nq"], injected["row_ptr"], 16
    H, G = _dense(n, d, d, False, 9300 + d), _dense(nq, d, d, False, 9400 + d, nan_row=EMPTY_ROW)
    try:
        for vt in (np.float32, np.float64):
            values = injected["values"][vt]
            for segs in (1, 3, 0):
                engine_test.set_option("prop_segs", segs)
                o32, o64, ps = engine_test.sparse_propagate(row_ptr, H, want64=True, values=values)
                _same(o64, o32, *_twin_fwd(injected, d, False, vt), ("fwd", vt, segs))
                assert ps["chunks"] == (ps["segments"] if segs == 1 else -(-ps["segments"] // 3) if segs == 3 else 1)
                o32, o64, ps = engine_test.sparse_propagate_t(row_ptr, G, want64=True, values=values)
                _same(o64, o32, *_twin_t(injected, d, False, vt), ("t", vt, segs))
                assert ps["chunks"] == (ps["segments"] if segs == 1 else -(-ps["segments"] // 3) if segs == 3 else 1)
    finally:
        engine_test.set_option("prop_segs", 0)


def test_the_transposition_is_built_once_and_plain_calls_keep_their_bits(engine_test, tiny, injected):
    _ensure_held(engine_test, tiny, injected)
    n, nq, row_ptr, ids, fix, d = injected["n"], injected["nq"], injected["row_ptr"], injected["ids"], injected["fix"], 16
    H, G = _dense(n, d, d, False, 9300 + d), _dense(nq, d, d, False, 9400 + d, nan_row=EMPTY_ROW)
    values = injected["values"][np.float32]
    want_v = _twin_t(injected, d, False, np.float32)
    key = ("plain", d)
    if key not in injected["twins"]:
        injected["twins"][key] = (pt.propagate_t_ref(row_ptr, ids, fix, G, n), pr.propagate_ref(row_ptr, ids, fix, H))
    plain_t, plain_f = injected["twins"][key]
    # ---- the values call is the first call after a hold: it builds the transposition
    injected["hold"]()
    o32, o64, ps = engine_test.sparse_propagate_t(row_ptr, G, want64=True, values=values)
    assert ps["built"] == 1 and ps["transpose_ms"] >= 0.0
    _same(o64, o32, *want_v, "values first")
    o32, o64, ps = engine_test.sparse_propagate_t(row_ptr, G, want64=True, values=values)
    assert ps["built"] == 0 and ps["transpose_ms"] == 0.0
    _same(o64, o32, *want_v, "values again")
    # a plain call after a values call: today's bits, nothing rebuilt
    o32, o64, ps = engine_test.sparse_propagate_t(row_ptr, G, want64=True)
    assert ps["built"] == 0
    _same(o64, o32, *plain_t, "plain after values")
    o32, o64, ps = engine_test.sparse_propagate(row_ptr, H, want64=True)
    _same(o64, o32, *plain_f, "plain forward after values")
    # ---- a values call after a plain call: the transposition is there, built == 0, the same bits
    injected["hold"]()
    o32, o64, ps = engine_test.sparse_propagate_t(row_ptr, G, want64=True)
    assert ps["built"] == 1
    _same(o64, o32, *plain_t, "plain first")
    o32, o64, ps = engine_test.sparse_propagate_t(row_ptr, G, want64=True, values=values)
    assert ps["built"] == 0 and ps["transpose_ms"] == 0.0 and ps["short_cols"] == ps["lds_cols"] == ps["global_cols"] == 0
    _same(o64, o32, *want_v, "values after plain")
    o32, o64, ps = engine_test.sparse_propagate_t(row_ptr, G, want64=True)
    assert ps["built"] == 0
    _same(o64, o32, *plain_t, "plain again")


def test_the_fetched_values_give_the_bits_of_the_plain_calls(engine_test, tiny, injected):
    _ensure_held(engine_test, tiny, injected)
    n, nq, row_ptr = injected["n"], injected["nq"], injected["row_ptr"]
    vals = injected["vals"]
    assert vals.dtype == np.float64 and (vals.view(np.uint64) == pr.weights(injected["fix"]).view(np.uint64)).all()
    for d, bf16 in ((5, False), (24, True)):
        H, G = _dense(n, d, d, bf16, 9500 + d), _dense(nq, d, d, bf16, 9600 + d, nan_row=EMPTY_ROW)
        p32, p64, _ = engine_test.sparse_propagate(row_ptr, H, bf16=bf16, want64=True)
        v32, v64, _ = engine_test.sparse_propagate(row_ptr, H, bf16=bf16, want64=True, values=vals)
        _same(v64, v32, p64, p32, ("fwd", d))
        p32, p64, _ = engine_test.sparse_propagate_t(row_ptr, G, bf16=bf16, want64=True)
        v32, v64, _ = engine_test.sparse_propagate_t(row_ptr, G, bf16=bf16, want64=True, values=vals)
        _same(v64, v32, p64, p32, ("t", d))


def _raw(engine, name, row_ptr, nq, feat, ftype, d, ldf, flags, values, vtype, out32, out64, ldo):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return getattr(engine._lib, name)(engine._ctx, p(row_ptr), C.c_int(nq), p(feat), C.c_int(ftype), C.c_int(d), C.c_int64(ldf), C.c_int(flags),
                                      p(values), C.c_int(vtype), p(out32), p(out64), C.c_int64(ldo), None)


def test_argument_errors(engine_test, tiny, injected):
    _ensure_held(engine_test, tiny, injected)
    n, nq, row_ptr, d = injected["n"], injected["nq"], injected["row_ptr"], 6
    v32, v64 = injected["values"][np.float32], injected["values"][np.float64]
    for name, rows_in, rows_out in (("fora_hip_sparse_propagate_vals", n, nq), ("fora_hip_sparse_propagate_t_vals", nq, n)):
        X = _dense(rows_in, d, d, False, 9700)
        o32, o64 = np.full((rows_out, d), -5.0, np.float32), np.full((rows_out, d), -5.0, np.float64)
        call = lambda flags, values, vtype: _raw(engine_test, name, row_ptr, nq, X, 0, d, d, flags, values, vtype, o32, o64, d)
        assert call(1, v32, 0) == -1                  # FORA_PROP_NORMALIZE together with values
        assert call(0, None, 0) == -1                 # NULL values while the held result has entries
        assert call(0, v32, 1) == -1                  # a bf16 val_type
        assert call(0, v32, 3) == -1 and call(0, v32, -1) == -1
        assert call(2, v32, 0) == -1                  # an unknown flag bit
        bad = row_ptr.copy()
        bad[-1] += 1
        assert _raw(engine_test, name, bad, nq, X, 0, d, d, 0, v32, 0, o32, o64, d) == -1
        assert _raw(engine_test, name, row_ptr, nq, X, 0, d, d - 1, 0, v32, 0, o32, o64, d) == -1
        assert _raw(engine_test, name, row_ptr, nq, X, 0, d, d, 0, v32, 0, None, None, d) == -1
        assert (o32 == -5.0).all() and (o64 == -5.0).all(), name                       # nothing was written
        assert call(0, v32, 0) == 0 and call(0, v64, 2) == 0                            # ... and both types are taken
        assert not (o64 == -5.0).any()
    with pytest.raises(ValueError):
        engine_test.sparse_propagate(row_ptr, _dense(n, d, d, False, 9700), values=v32[:-1])      # one element per entry
    with pytest.raises(ValueError):
        engine_test.sparse_propagate(row_ptr, _dense(n, d, d, False, 9700), values=np.zeros(len(v32), np.float16))
    engine_test.sparse_clear()
    X = _dense(n, d, d, False, 9700)
    o32 = np.full((nq, d), -5.0, np.float32)
    assert _raw(engine_test, "fora_hip_sparse_propagate_vals", row_ptr, nq, X, 0, d, d, 0, v32, 0, o32, None, d) == -1     # no held result
    assert (o32 == -5.0).all()
    injected["hold"]()


def test_the_three_operations_are_adjoint_on_exact_data(engine_test, tiny, injected):
    """with A, B and g small integers stored as f32 every f64 sum is exact, so sum_e g_e sddmm(A, B)_e,
    sum A * propagate_vals(g, B) and sum B * propagate_t_vals(g, A) are one integer: a check that leans on no twin"""
    _ensure_held(engine_test, tiny, injected)
    n, nq, row_ptr, e = injected["n"], injected["nq"], injected["row_ptr"], injected["entries"]
    rng = np.random.Generator(np.random.PCG64(9800))
    for d in (7, 70):
        A = rng.integers(-9, 10, size=(nq, d)).astype(np.float32)
        B = rng.integers(-9, 10, size=(n, d)).astype(np.float32)
        g = rng.integers(-9, 10, size=e).astype(np.float32)
        _, s64, _ = engine_test.sparse_sddmm(row_ptr, A, B, want32=False, want64=True)
        _, f64, _ = engine_test.sparse_propagate(row_ptr, B, want32=False, want64=True, values=g)
        _, t64, _ = engine_test.sparse_propagate_t(row_ptr, A, want32=False, want64=True, values=g)
        ints = lambda x: [int(v) for v in np.asarray(x, dtype=np.float64).ravel()]
        for x in (s64, f64, t64):
            assert (x == np.rint(x)).all() and np.abs(x).max() < 2.0 ** 40
        one = sum(a * b for a, b in zip(ints(g), ints(s64)))
        two = sum(a * b for a, b in zip(ints(A), ints(f64)))
        three = sum(a * b for a, b in zip(ints(B), ints(t64)))
        assert one == two == three and one != 0, (d, one, two, three)
