"""PROPAGATE, TRANSPOSED (fora_hip_sparse_propagate_t, fora_hip_sparse_transpose_fetch) on the GPU: the transposition of the
held sparse rows word for word against a stable sort, and its product with a gradient bit for bit against the numpy twin of
the contract (tests/propagate_t_ref.py).  Every bit-order assertion is made on out64; out32 is checked as (float)out64."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import propagate_ref as pr
import propagate_t_ref as pt
from test_sparse_gpu import SEED, _mixed_sources, _raw_fetch

pytestmark = pytest.mark.gpu
CAPS = (0, 64, pt.LDS_MAX)                     # "propt_lds_cap": every run global, medium runs global, the default


def _load(engine, g, **kw):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(seed=SEED, epsilon=0.5, **kw)


@pytest.fixture(scope="module")
def injected(engine_test, tiny):
    """the held result of the injected rows (columns of chosen lengths) on the test build's engine, its fetched arrays and
    its transposition by the twin -- made once, never changed"""
    _load(engine_test, tiny)
    rows_fix, col_lens = pt.injected_columns(tiny.n)
    want_ptr, want_ids, want_fix = pt.csr_of(rows_fix)
    held = {"n": tiny.n, "nq": rows_fix.shape[0], "col_lens": col_lens}

    def hold():
        row_ptr, sp = engine_test.test_sparse_rows(rows_fix, threshold=0.0)
        assert (row_ptr == want_ptr).all() and row_ptr[300] == row_ptr[301]
        e = int(row_ptr[-1])
        ids, fix = np.zeros(e, np.int32), np.zeros(e, np.uint64)
        assert _raw_fetch(engine_test, ids, None, fix, e) == 0
        assert (ids == want_ids).all() and (fix == want_fix).all()
        held.update(row_ptr=row_ptr, ids=ids, fix=fix)
    held["hold"] = hold
    hold()
    held["col_ptr"], held["rows"], held["fix_t"] = pt.transpose_ref(held["row_ptr"], held["ids"], held["fix"], tiny.n)
    assert (np.diff(held["col_ptr"]) == col_lens).all()
    held["twins"] = {}
    return held


def _ensure_held(engine_test, tiny, injected):
    """another module may have used the session's test engine in between: put graph and rows back if so"""
    e = int(injected["row_ptr"][-1])
    ids = np.zeros(e, np.int32)
    if engine_test.n != tiny.n or _raw_fetch(engine_test, ids, None, None, e) != 0 or not (ids == injected["ids"]).all():
        _load(engine_test, tiny)
        injected["hold"]()
    engine_test.set_option("propt_lds_cap", pt.LDS_MAX)
    engine_test.set_option("prop_segs", 0)


def _gradient(nq, d, ldg, bf16, seed, nan_row=None):
    """[nq, d] gradients as a view of an [nq, ldg] array (the padding holds NaN patterns that must never be read into a sum);
    nan_row: a row of NaN -- the row of G that belongs to an empty held row"""
    rng = np.random.Generator(np.random.PCG64(seed))
    G = pr.scaled_features(rng, nq, d)
    if bf16:
        wide = np.full((nq, ldg), 0x7FC1, dtype=np.uint16)
        wide[:, :d] = pr.to_bf16_bits(G)
        if nan_row is not None:
            wide[nan_row] = 0x7FC1
    else:
        wide = np.full((nq, ldg), np.nan, dtype=np.float32)
        wide[:, :d] = G
        if nan_row is not None:
            wide[nan_row] = np.nan
    return wide[:, :d]


def _twin(injected, d, bf16, normalize, seed):
    key = (d, bf16, normalize, seed)
    if key not in injected["twins"]:
        G = _gradient(injected["nq"], d, d, bf16, seed, nan_row=300)
        injected["twins"][key] = pt.propagate_t_ref(injected["row_ptr"], injected["ids"], injected["fix"], G, injected["n"], normalize=normalize, bf16=bf16)
    return injected["twins"][key]


def _same(got64, got32, want64, want32, what):
    assert (got64.view(np.uint64) == want64.view(np.uint64)).all(), what
    assert (got32.view(np.uint32) == want32.view(np.uint32)).all(), what
    assert (got32.view(np.uint32) == got64.astype(np.float32).view(np.uint32)).all(), what


def test_transposition_equals_the_stable_sort(engine_test, tiny, injected):
    """an integer check of the new kernels with no floating point in it, on every sort tier"""
    _ensure_held(engine_test, tiny, injected)
    row_ptr = injected["row_ptr"]
    try:
        for cap in CAPS:
            engine_test.set_option("propt_lds_cap", cap)
            col_ptr, rows, vals, fix = engine_test.sparse_transpose_fetch(row_ptr, want_fix=True)
            assert col_ptr.dtype == np.int64 and rows.dtype == np.int32 and fix.dtype == np.uint64 and vals.dtype == np.float64
            assert (col_ptr == injected["col_ptr"]).all(), cap
            assert (rows == injected["rows"]).all(), cap
            assert (fix == injected["fix_t"]).all(), cap
            assert (vals.view(np.uint64) == pr.weights(injected["fix_t"]).view(np.uint64)).all(), cap
        # every pointer may be NULL; a cap below the held entries writes nothing
        e = int(row_ptr[-1])
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        fetch = engine_test._lib.fora_hip_sparse_transpose_fetch
        only_rows = np.full(e, -9, np.int32)
        assert fetch(engine_test._ctx, p(row_ptr), C.c_int(len(row_ptr) - 1), None, p(only_rows), None, None, C.c_uint64(e)) == 0
        assert (only_rows == injected["rows"]).all()
        assert fetch(engine_test._ctx, p(row_ptr), C.c_int(len(row_ptr) - 1), None, None, None, None, C.c_uint64(e)) == 0
        only_rows[:] = -9
        assert fetch(engine_test._ctx, p(row_ptr), C.c_int(len(row_ptr) - 1), None, p(only_rows), None, None, C.c_uint64(e - 1)) == -1
        assert (only_rows == -9).all()
    finally:
        engine_test.set_option("propt_lds_cap", pt.LDS_MAX)


@pytest.mark.parametrize("d", [1, 3, 16, 65, 130])
def test_injected_columns_equal_the_twin(engine_test, tiny, injected, d):
    _ensure_held(engine_test, tiny, injected)
    n, nq, row_ptr = injected["n"], injected["nq"], injected["row_ptr"]
    for bf16 in (False, True):
        elt = 2 if bf16 else 4
        for ldg in (d, d + 3):
            G = _gradient(nq, d, ldg, bf16, 7200 + d, nan_row=300)       # the same values at every pitch
            assert G.strides[0] == ldg * elt
            for normalize in (False, True):
                want64, want32 = _twin(injected, d, bf16, normalize, 7200 + d)
                assert np.isfinite(want64).all()                          # row 300 of G, all NaN, reaches no output
                for ldo in (d, d + 5):
                    o32 = np.full((n, ldo), -77.0, dtype=np.float32)
                    o64 = np.full((n, ldo), -77.0, dtype=np.float64)
                    _, _, ps = engine_test.sparse_propagate_t(row_ptr, G, normalize=normalize, bf16=bf16, out32=o32[:, :d], out64=o64[:, :d])
                    what = (d, bf16, ldg, normalize, ldo)
                    _same(o64[:, :d], o32[:, :d], want64, want32, what)
                    assert (o32[:, d:] == -77.0).all() and (o64[:, d:] == -77.0).all(), what      # the padding survives
                    ref = pt.propt_stats_ref(injected["col_ptr"], d, elt)
                    assert {k: ps[k] for k in ref} == ref and ps["feat_on_device"] == 0 and ps["chunks"] >= 1, what
                    assert ps["gather_ms"] >= 0.0 and ps["combine_ms"] >= 0.0
        # one output at a time
        G = _gradient(nq, d, d, bf16, 7200 + d, nan_row=300)
        a32, a64, _ = engine_test.sparse_propagate_t(row_ptr, G, bf16=bf16, want32=True, want64=False)
        b32, b64, _ = engine_test.sparse_propagate_t(row_ptr, G, bf16=bf16, want32=False, want64=True)
        want64, want32 = _twin(injected, d, bf16, False, 7200 + d)
        assert a64 is None and b32 is None and a32.shape == b64.shape == (n, d)
        assert (b64.view(np.uint64) == want64.view(np.uint64)).all() and (a32.view(np.uint32) == want32.view(np.uint32)).all()
    empty = np.flatnonzero(injected["col_lens"] == 0)
    assert empty.size >= 3 and (want64[empty] == 0.0).all() and not np.signbit(b64[empty]).any()   # a node no row keeps: +0.0


def test_lds_cap_changes_no_bit(engine_test, tiny, injected):
    _ensure_held(engine_test, tiny, injected)
    row_ptr, nq, d = injected["row_ptr"], injected["nq"], 16
    G = _gradient(nq, d, d, False, 7300, nan_row=300)
    try:
        for normalize in (False, True):
            want64, want32 = _twin(injected, d, False, normalize, 7300)
            engine_test.set_option("propt_lds_cap", pt.LDS_MAX)
            for cap in CAPS:
                engine_test.set_option("propt_lds_cap", cap)                 # a change drops the cached transposition
                assert engine_test.get_option("propt_lds_cap") == cap
                o32, o64, ps = engine_test.sparse_propagate_t(row_ptr, G, normalize=normalize, want64=True)
                _same(o64, o32, want64, want32, (cap, normalize))
                tiers = pt.tier_counts(injected["col_ptr"], cap)           # (every cap of CAPS differs from the one before it)
                assert ps["built"] == 1 and {k: ps[k] for k in tiers} == tiers and ps["transpose_ms"] >= 0.0, (cap, ps)
                # the same value again: no change, the transposition stays
                engine_test.set_option("propt_lds_cap", cap)
                o32, o64, ps = engine_test.sparse_propagate_t(row_ptr, G, normalize=normalize, want64=True)
                _same(o64, o32, want64, want32, (cap, normalize, "again"))
                assert ps["built"] == 0 and ps["transpose_ms"] == 0.0 and ps["short_cols"] == ps["lds_cols"] == ps["global_cols"] == 0
        # every tier was reached by some setting
        lens = injected["col_lens"]
        assert pt.tier_counts(injected["col_ptr"], 0)["global_cols"] == int((lens >= 2).sum())
        assert pt.tier_counts(injected["col_ptr"], 64) == {"short_cols": int(((lens >= 2) & (lens <= 64)).sum()), "lds_cols": 0, "global_cols": int((lens > 64).sum())}
        assert pt.tier_counts(injected["col_ptr"])["lds_cols"] == int((lens > 64).sum()) >= 24    # (eight of COL_LENS, three nodes each)
    finally:
        engine_test.set_option("propt_lds_cap", pt.LDS_MAX)


def test_prop_segs_changes_no_bit(engine_test, tiny, injected):
    _ensure_held(engine_test, tiny, injected)
    row_ptr, nq, d = injected["row_ptr"], injected["nq"], 20
    G = _gradient(nq, d, d, False, 7400, nan_row=300)
    segments = pt.propt_stats_ref(injected["col_ptr"], d, 4)["segments"]
    assert segments > 3
    try:
        for normalize in (False, True):
            want64, want32 = _twin(injected, d, False, normalize, 7400)
            for segs, chunks in ((1, segments), (3, -(-segments // 3)), (0, 1)):
                engine_test.set_option("prop_segs", segs)
                o32, o64, ps = engine_test.sparse_propagate_t(row_ptr, G, normalize=normalize, want64=True)
                assert ps["chunks"] == chunks and ps["segments"] == segments, (segs, ps)
                _same(o64, o32, want64, want32, (segs, normalize))
    finally:
        engine_test.set_option("prop_segs", 0)


def _check_held(engine, row_ptr, ids, fix, n, seed, cases):
    """both new calls on the held result against the twin fed with the fetched (ids, fix)"""
    nq = len(row_ptr) - 1
    col_ptr, rows, fix_t = pt.transpose_ref(row_ptr, ids, fix, n)
    g_ptr, g_rows, g_vals, g_fix = engine.sparse_transpose_fetch(row_ptr, want_fix=True)
    assert (g_ptr == col_ptr).all() and (g_rows == rows).all() and (g_fix == fix_t).all()
    for d, bf16, normalize in cases:
        G = _gradient(nq, d, d + (1 if d % 2 else 0), bf16, seed + d)
        want64, want32 = pt.propagate_t_ref(row_ptr, ids, fix, G, n, normalize=normalize, bf16=bf16)
        o32, o64, ps = engine.sparse_propagate_t(row_ptr, G, normalize=normalize, bf16=bf16, want64=True)
        _same(o64, o32, want64, want32, (d, bf16, normalize))
        ref = pt.propt_stats_ref(col_ptr, d, 2 if bf16 else 4)
        assert {k: ps[k] for k in ref} == ref


@pytest.mark.parametrize("gname", ["tiny_dangling", "small"])
def test_real_rows_equal_the_twin(engine, request, gname):
    g = request.getfixturevalue(gname)
    srcs = _mixed_sources(g, 7500)                # a duplicate, and on tiny_dangling a dangling source
    assert int((g.deg[srcs] == 0).sum()) == (1 if gname == "tiny_dangling" else 0)
    _load(engine, g)
    try:
        for with_idx in (False, True):
            if with_idx:
                engine.build_index()
            for t, cases in ((0.0, [(5, False, False), (5, False, True)]), (1.0 / g.n, [(8, True, True), (3, False, False)])):
                row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, with_idx=with_idx, threshold=t, want_fix=True)
                _check_held(engine, row_ptr, ids, fix, g.n, 7500, cases)
        live = [int(s) for s in srcs if g.deg[s] > 0]
        sets = [live[:3], live[2:5], [int(srcs[3])] + live[:1]]
        for weights in (None, [[0.5, 0.25, 0.25], [3.0, 1.0, 2.0], [1.0, 7.0]]):
            r = engine.query_seeds_sparse(sets, weights, threshold=1.0 / g.n, want_fix=True)
            _check_held(engine, r["row_ptr"], r["ids"], r["fix"], g.n, 7550, [(6, False, True), (4, True, False)])
    finally:
        engine.clear_index()


@pytest.mark.parametrize("gname", ["tiny_dangling", "small"])
def test_identity_gradient_gives_the_dense_words(engine, request, gname):
    """a yardstick that is not the twin: with G the nq x nq identity, out64[v][i] is exactly the dense row i's word at v times
    2^-62 where it passes the threshold, and +0.0 elsewhere -- every sum has one non-zero term"""
    from test_sparse_gpu import thr_fix_of
    g = request.getfixturevalue(gname)
    _load(engine, g)
    srcs = _mixed_sources(g, 7600)
    nq = len(srcs)
    dense, _, _ = engine.query_fix(srcs, want_residue=False)
    G = np.eye(nq, dtype=np.float32)
    for t in (0.0, 1.0 / g.n):
        thr = np.uint64(thr_fix_of(t))
        row_ptr, ids, vals, st, sp = engine.query_sparse(srcs, threshold=t)
        o32, o64, ps = engine.sparse_propagate_t(row_ptr, G, want64=True)
        want = np.where(dense >= thr, np.ldexp(dense.astype(np.float64), -62), 0.0).T
        assert o64.shape == (g.n, nq) and (o64.view(np.uint64) == np.ascontiguousarray(want).view(np.uint64)).all()
        assert (want > 0).sum() == sp["entries"] and (o32 == want.astype(np.float32)).all()


def test_state_is_left_alone_and_the_transposition_follows_the_held_result(engine, small):
    g = small
    _load(engine, g)
    srcs = _mixed_sources(g, 7700)
    nq = len(srcs)
    sw = engine.sweep(srcs[:3], want_profile=True)
    gen0 = engine.get_option("sparse_generation")
    row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, want_fix=True)
    gen1 = engine.get_option("sparse_generation")
    assert gen1 > gen0
    params, batch, e = engine.get_params(), engine.get_batch(), sp["entries"]
    H = pr.scaled_features(np.random.Generator(np.random.PCG64(7701)), g.n, 10)
    _, fwd_before, _ = engine.sparse_propagate(row_ptr, H, want32=False, want64=True, normalize=True)
    engine.reset_timing()
    t0 = engine.timing()
    G = _gradient(nq, 10, 10, False, 7702)
    want64, want32 = pt.propagate_t_ref(row_ptr, ids, fix, G, g.n)
    o32, o64, ps = engine.sparse_propagate_t(row_ptr, G, want64=True)
    assert ps["built"] == 1
    _same(o64, o32, want64, want32, "first")
    o32, o64, ps = engine.sparse_propagate_t(row_ptr, G, want64=True)          # a second call: the cached transposition, the same bits
    assert ps["built"] == 0 and ps["transpose_ms"] == 0.0
    _same(o64, o32, want64, want32, "second")
    engine.sparse_transpose_fetch(row_ptr)
    _, fwd_after, _ = engine.sparse_propagate(row_ptr, H, want32=False, want64=True, normalize=True)
    assert (fwd_after.view(np.uint64) == fwd_before.view(np.uint64)).all()     # the forward product, before and after
    i2, v2, f2 = np.zeros(e, np.int32), np.zeros(e, np.float64), np.zeros(e, np.uint64)
    assert _raw_fetch(engine, i2, v2, f2, e) == 0 and (i2 == ids).all() and (v2 == vals).all() and (f2 == fix).all()
    assert engine.timing() == t0 and engine.get_params() == params and engine.get_batch() == batch
    assert engine.get_option("sparse_generation") == gen1                      # neither call moves it
    ids_s, cut_s, vol_s = engine.sweep_fetch(int(sw["row_ptr"][-1]))           # the held sweep profile survives
    assert (ids_s == sw["ids"]).all() and (cut_s == sw["cut"]).all() and (vol_s == sw["vol"]).all()
    # a new query_sparse: the generation moves, the next call builds again, on the new rows
    row_ptr2, ids2, vals2, fix2, st, sp = engine.query_sparse(srcs[:4], threshold=1e-3, want_fix=True)
    assert engine.get_option("sparse_generation") > gen1
    G2 = _gradient(4, 10, 10, False, 7703)
    want64, want32 = pt.propagate_t_ref(row_ptr2, ids2, fix2, G2, g.n)
    o32, o64, ps = engine.sparse_propagate_t(row_ptr2, G2, want64=True)
    assert ps["built"] == 1 and ps["entries"] == sp["entries"]
    _same(o64, o32, want64, want32, "rebuilt")
    # after sparse_clear both calls refuse
    gen2 = engine.get_option("sparse_generation")
    engine.sparse_clear()
    assert engine.get_option("sparse_generation") > gen2
    from fora_amd import ForaError
    with pytest.raises(ForaError) as err:
        engine.sparse_propagate_t(row_ptr2, G2)
    assert err.value.code == -1
    with pytest.raises(ForaError) as err:
        engine.sparse_transpose_fetch(row_ptr2)
    assert err.value.code == -1


def _raw(engine, row_ptr, nq, grad, gtype, d, ldg, flags, out32, out64, ldo):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return engine._lib.fora_hip_sparse_propagate_t(engine._ctx, p(row_ptr), C.c_int(nq), p(grad), C.c_int(gtype), C.c_int(d), C.c_int64(ldg),
                                                   C.c_int(flags), p(out32), p(out64), C.c_int64(ldo), None)


def test_argument_errors(engine, tiny):
    g = tiny
    _load(engine, g)
    srcs = _mixed_sources(g, 7800)
    d, nq = 6, len(srcs)
    G = _gradient(nq, d, d, False, 7801)
    o32, o64 = np.full((g.n, d), -5.0, np.float32), np.full((g.n, d), -5.0, np.float64)
    engine.sparse_clear()
    rp0 = np.zeros(nq + 1, np.int64)
    assert _raw(engine, rp0, nq, G, 0, d, d, 0, o32, o64, d) == -1                    # no held result
    row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, want_fix=True)
    e = sp["entries"]
    end, dec, first, short = row_ptr.copy(), row_ptr.copy(), row_ptr.copy(), row_ptr.copy()
    end[-1] += 1
    dec[2] = dec[1] - 1
    first[0] = 1
    short[-1] -= 1
    for bad in (end, short, dec, first):
        assert _raw(engine, bad, nq, G, 0, d, d, 0, o32, o64, d) == -1
    assert _raw(engine, None, nq, G, 0, d, d, 0, o32, o64, d) == -1
    assert _raw(engine, row_ptr, -1, G, 0, d, d, 0, o32, o64, d) == -1
    assert _raw(engine, row_ptr, nq, None, 0, d, d, 0, o32, o64, d) == -1             # NULL grad with entries to read
    assert _raw(engine, row_ptr, nq, G, 0, d, d - 1, 0, o32, o64, d) == -1            # ldg < d
    assert _raw(engine, row_ptr, nq, G, 0, d, d, 0, o32, o64, d - 1) == -1            # ldo < d
    assert _raw(engine, row_ptr, nq, G, 0, 0, d, 0, o32, o64, d) == -1                # d = 0
    assert _raw(engine, row_ptr, nq, G, 0, 65537, 65537, 0, o32, o64, 65537) == -1
    assert _raw(engine, row_ptr, nq, G, 0, d, d, 0, None, None, d) == -1              # both outputs NULL
    assert _raw(engine, row_ptr, nq, G, 2, d, d, 0, o32, o64, d) == -1                # a bad grad_type
    assert _raw(engine, row_ptr, nq, G, -1, d, d, 0, o32, o64, d) == -1
    assert _raw(engine, row_ptr, nq, G, 0, d, d, 2, o32, o64, d) == -1                # an unknown flag bit
    assert (o32 == -5.0).all() and (o64 == -5.0).all()                                # nothing was written
    i2, f2 = np.zeros(e, np.int32), np.zeros(e, np.uint64)
    assert _raw_fetch(engine, i2, None, f2, e) == 0 and (i2 == ids).all() and (f2 == fix).all()   # the held result is intact
    assert _raw(engine, row_ptr, nq, G, 0, d, d, 0, o32, o64, d) == 0                 # ... and usable
    want64, want32 = pt.propagate_t_ref(row_ptr, ids, fix, G, g.n)
    _same(o64, o32, want64, want32, "after the errors")
    # the binding refuses what the C ABI cannot express
    with pytest.raises(ValueError):
        engine.sparse_propagate_t(row_ptr, np.zeros((nq, 2 * d), np.float32)[:, ::2])  # a column stride of two elements
    with pytest.raises(ValueError):
        engine.sparse_propagate_t(row_ptr, np.zeros((g.n, d), np.float32))              # [n, d]: the forward call's shape
    with pytest.raises(ValueError):
        engine.sparse_propagate_t(row_ptr, np.zeros((nq, d), np.float64))
    # nq == 0, an empty held result: FORA_OK with a NULL grad, every output +0.0
    engine.query_sparse(np.zeros(0, np.int32))
    o32[:] = -5.0
    assert _raw(engine, np.zeros(1, np.int64), 0, None, 0, d, d, 0, o32, None, d) == 0
    assert (o32 == 0.0).all() and not np.signbit(o32).any()


def test_device_pointers_and_autograd():
    """grad and the outputs as torch tensors on the GPU, and fora_amd.torch_ops.ppr_propagate's backward pass, in a fresh
    child process (tests/propagate_t_device_child.py): torch and the library must live on one HIP runtime, so the child
    imports torch before the library is loaded."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "propagate_t_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "propagate_t device ok" in r.stdout
