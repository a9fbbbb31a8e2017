"""SCORES (SDDMM) (fora_hip_sparse_sddmm) on the GPU: one dot product per held entry, bit for bit against the numpy twin of the
contract (tests/sddmm_ref.py).  Every bit-order assertion is made on out64; out32 is checked as (float)out64.  The features
are scaled over 2^+-20 (propagate_ref.scaled_features), so another order of the additions changes bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import propagate_ref as pr
import sddmm_ref as sr
from test_sparse_gpu import SEED, _mixed_sources, _raw_fetch

pytestmark = pytest.mark.gpu
ROW_LENS, EMPTY, injected_rows, operand = sr.ROW_LENS, sr.EMPTY, sr.injected_rows, sr.operand
WIDTHS = [1, 3, 63, 64, 65, 130, 200]
TYPES = [(False, False), (False, True), (True, False), (True, True)]


def _load(engine, g, **kw):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(seed=SEED, epsilon=0.5, **kw)


@pytest.fixture(scope="module")
def held(engine_test, tiny):
    """the held result of the injected rows on the test build's engine and its fetched ids -- made once, never changed"""
    _load(engine_test, tiny)
    rows_fix = injected_rows(tiny.n)
    h = {"n": tiny.n, "nq": len(ROW_LENS), "twins": {}}

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


def _ensure_held(engine_test, tiny, held):
    """another module may have used the session's test engine in between: put graph and rows back if so"""
    e = held["entries"]
    ids = np.zeros(e, np.int32)
    if engine_test.n != tiny.n or _raw_fetch(engine_test, ids, None, None, e) != 0 or not (ids == held["ids"]).all():
        _load(engine_test, tiny)
        held["hold"]()
    engine_test.set_option("prop_segs", 0)


def _twin(held, d, a_bf16, b_bf16):
    key = (d, a_bf16, b_bf16)
    if key not in held["twins"]:
        A = operand(held["nq"], d, d, a_bf16, 8700 + d, nan_row=EMPTY)
        B = operand(held["n"], d, d, b_bf16, 8800 + d)
        held["twins"][key] = sr.sddmm_ref(held["row_ptr"], held["ids"], A, B, a_bf16=a_bf16, b_bf16=b_bf16)
    return held["twins"][key]


def _same(got64, got32, want64, want32, what):
    assert (got64.view(np.uint64) == want64.view(np.uint64)).all(), what
    assert (got32.view(np.uint32) == want32.view(np.uint32)).all(), what
    assert (got32.view(np.uint32) == got64.astype(np.float32).view(np.uint32)).all(), what


@pytest.mark.parametrize("d", WIDTHS)
def test_injected_rows_equal_the_twin(engine_test, tiny, held, d):
    _ensure_held(engine_test, tiny, held)
    n, nq, row_ptr, e = held["n"], held["nq"], held["row_ptr"], held["entries"]
    pitches = [(d, d), (d + 3, d + 7)] if d != 200 else [(d + 3, d + 7)]       # odd pitches: no row but the first is aligned
    for a_bf16, b_bf16 in TYPES:
        want64, want32 = _twin(held, d, a_bf16, b_bf16)
        assert np.isfinite(want64).all()                                        # the NaN row of a and the padding reach no score
        for lda, ldb in pitches:
            A = operand(nq, d, lda, a_bf16, 8700 + d, nan_row=EMPTY)
            B = operand(n, d, ldb, b_bf16, 8800 + d)
            o32, o64, st = engine_test.sparse_sddmm(row_ptr, A, B, want64=True, a_bf16=a_bf16, b_bf16=b_bf16)
            what = (d, a_bf16, b_bf16, lda, ldb)
            assert o32.shape == o64.shape == (e,)
            _same(o64, o32, want64, want32, what)
            ref = sr.sddmm_stats_ref(row_ptr, d, 2 if a_bf16 else 4, 2 if b_bf16 else 4)
            assert {k: st[k] for k in ref} == ref and st["a_on_device"] == 0 and st["b_on_device"] == 0 and st["sddmm_ms"] >= 0.0, what
    # one output at a time, and a caller-made output longer than the entries keeps its tail
    A, B = operand(nq, d, d, False, 8700 + d, nan_row=EMPTY), operand(n, d, d, False, 8800 + d)
    want64, want32 = _twin(held, d, False, False)
    a32, a64, _ = engine_test.sparse_sddmm(row_ptr, A, B, want32=True, want64=False)
    b32, b64, _ = engine_test.sparse_sddmm(row_ptr, A, B, want32=False, want64=True)
    assert a64 is None and b32 is None
    assert (b64.view(np.uint64) == want64.view(np.uint64)).all() and (a32.view(np.uint32) == want32.view(np.uint32)).all()
    long64 = np.full(e + 4, -77.0, dtype=np.float64)
    engine_test.sparse_sddmm(row_ptr, A, B, want32=False, out64=long64)
    assert (long64[:e].view(np.uint64) == want64.view(np.uint64)).all() and (long64[e:] == -77.0).all()


def test_batch_and_prop_segs_change_no_bit(engine_test, tiny, held):
    _ensure_held(engine_test, tiny, held)
    n, nq, row_ptr = held["n"], held["nq"], held["row_ptr"]
    try:
        for d in (3, 130):
            A, B = operand(nq, d, d, False, 8700 + d, nan_row=EMPTY), operand(n, d, d, True, 8800 + d)
            want64, want32 = _twin(held, d, False, True)
            for b, segs in ((1, 1), (7, 3), (0, 0)):
                engine_test.set_batch(b)
                engine_test.set_option("prop_segs", segs)
                o32, o64, st = engine_test.sparse_sddmm(row_ptr, A, B, want64=True, b_bf16=True)
                _same(o64, o32, want64, want32, (d, b, segs))
    finally:
        engine_test.set_batch(0)                     # (the request a fresh context has)
        engine_test.set_option("prop_segs", 0)


def _check_held(engine, row_ptr, ids, n, seed, cases):
    nq = len(row_ptr) - 1
    for d, a_bf16, b_bf16 in cases:
        A, B = operand(nq, d, d + 1, a_bf16, seed + d), operand(n, d, d, b_bf16, seed + 50 + d)
        want64, want32 = sr.sddmm_ref(row_ptr, ids, A, B, a_bf16=a_bf16, b_bf16=b_bf16)
        o32, o64, st = engine.sparse_sddmm(row_ptr, A, B, want64=True, a_bf16=a_bf16, b_bf16=b_bf16)
        _same(o64, o32, want64, want32, (d, a_bf16, b_bf16))
        assert st["entries"] == len(ids)


def test_real_held_results_equal_the_twin(engine, tiny_dangling):
    """the held result of a query, of a top-k query and of a seed-set call work as the injected rows do"""
    g = tiny_dangling
    srcs = _mixed_sources(g, 8900)                # a duplicate and a dangling source
    _load(engine, g)
    row_ptr, ids, vals, st, sp = engine.query_sparse(srcs, threshold=0.0)
    _check_held(engine, row_ptr, ids, g.n, 8900, [(5, False, False), (70, True, False)])
    row_ptr, ids, vals, st, sp, tk = engine.query_sparse_topk(srcs, 32, threshold=0.0)
    assert int(np.diff(row_ptr).max()) == 32
    _check_held(engine, row_ptr, ids, g.n, 8910, [(16, False, True), (64, False, False)])
    live = [int(s) for s in srcs if g.deg[s] > 0]
    r = engine.query_seeds_sparse([live[:3], live[2:5]], [[0.5, 0.25, 0.25], [3.0, 1.0, 2.0]], threshold=1.0 / g.n)
    _check_held(engine, r["row_ptr"], r["ids"], g.n, 8920, [(6, True, True), (33, False, False)])


def _raw(engine, row_ptr, nq, a, at, lda, b, bt, ldb, d, o32, o64, cap):
    p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    return engine._lib.fora_hip_sparse_sddmm(engine._ctx, p(row_ptr), C.c_int(nq), p(a), C.c_int(at), C.c_int64(lda), p(b), C.c_int(bt), C.c_int64(ldb),
                                             C.c_int(d), p(o32), p(o64), C.c_uint64(cap), None)


def test_argument_errors(engine, tiny):
    g = tiny
    _load(engine, g)
    srcs = _mixed_sources(g, 9000)
    d, nq = 6, len(srcs)
    A, B = operand(nq, d, d, False, 9001), operand(g.n, d, d, False, 9002)
    engine.sparse_clear()
    rp0 = np.zeros(nq + 1, np.int64)
    big = 1 << 20
    o32, o64 = np.full(big, -5.0, np.float32), np.full(big, -5.0, np.float64)
    assert _raw(engine, rp0, nq, A, 0, d, B, 0, d, d, o32, o64, big) == -1             # no held result
    row_ptr, ids, vals, st, sp = engine.query_sparse(srcs, threshold=1.0 / g.n)
    e = sp["entries"]
    assert 0 < e <= big
    end, dec, first, short = row_ptr.copy(), row_ptr.copy(), row_ptr.copy(), row_ptr.copy()
    end[-1] += 1
    dec[2] = dec[1] - 1
    first[0] = 1
    short[-1] -= 1
    for bad in (end, short, dec, first):
        assert _raw(engine, bad, nq, A, 0, d, B, 0, d, d, o32, o64, big) == -1          # a row_ptr that is not the held result's
    assert _raw(engine, None, nq, A, 0, d, B, 0, d, d, o32, o64, big) == -1
    assert _raw(engine, row_ptr, -1, A, 0, d, B, 0, d, d, o32, o64, big) == -1
    assert _raw(engine, row_ptr, nq, A, 0, d, B, 0, d, d, o32, o64, e - 1) == -1        # cap too small
    assert _raw(engine, row_ptr, nq, A, 0, d, B, 0, d, d, None, None, big) == -1        # both outputs NULL
    assert _raw(engine, row_ptr, nq, A, 0, d, B, 0, d, 0, o32, o64, big) == -1          # d = 0
    assert _raw(engine, row_ptr, nq, A, 0, 65537, B, 0, 65537, 65537, o32, o64, big) == -1
    assert _raw(engine, row_ptr, nq, A, 0, d - 1, B, 0, d, d, o32, o64, big) == -1      # a pitch below d
    assert _raw(engine, row_ptr, nq, A, 0, d, B, 0, d - 1, d, o32, o64, big) == -1
    assert _raw(engine, row_ptr, nq, A, 2, d, B, 0, d, d, o32, o64, big) == -1          # an unknown type (f64 is for values only)
    assert _raw(engine, row_ptr, nq, A, 0, d, B, -1, d, d, o32, o64, big) == -1
    assert _raw(engine, row_ptr, nq, None, 0, d, B, 0, d, d, o32, o64, big) == -1       # NULL operands with entries to read
    assert _raw(engine, row_ptr, nq, A, 0, d, None, 0, d, d, o32, o64, big) == -1
    assert (o32 == -5.0).all() and (o64 == -5.0).all()                                  # nothing was written
    i2 = np.zeros(e, np.int32)
    assert _raw_fetch(engine, i2, None, None, e) == 0 and (i2 == ids).all()              # the held result is intact
    assert _raw(engine, row_ptr, nq, A, 0, d, B, 0, d, d, o32, o64, e) == 0              # ... and usable
    want64, want32 = sr.sddmm_ref(row_ptr, ids, A, B)
    _same(o64[:e], o32[:e], want64, want32, "after the errors")
    assert (o32[e:] == -5.0).all() and (o64[e:] == -5.0).all()
    # the binding refuses what the C ABI cannot express
    with pytest.raises(ValueError):
        engine.sparse_sddmm(row_ptr, A, np.zeros((g.n, d + 1), np.float32))               # two widths
    with pytest.raises(ValueError):
        engine.sparse_sddmm(row_ptr, np.zeros((g.n, d), np.float32), B)                   # a is [nq, d]
    with pytest.raises(ValueError):
        engine.sparse_sddmm(row_ptr, A, B.astype(np.float64))
    # nq == 0, an empty held result: FORA_OK, nothing written
    engine.query_sparse(np.zeros(0, np.int32))
    o32[:] = -5.0
    assert _raw(engine, np.zeros(1, np.int64), 0, None, 0, d, None, 0, d, d, o32, None, 0) == 0
    assert (o32 == -5.0).all()


def test_device_operands_and_outputs():
    """a, b and the outputs as torch tensors on the GPU -- b also as a column slice that starts at an odd element -- in a
    fresh child process (tests/sddmm_device_child.py): torch and the library must live on one HIP runtime, so the child
    imports torch before the library is loaded."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "sddmm_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "sddmm device ok" in r.stdout
