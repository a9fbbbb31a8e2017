"""ROW SOFTMAX (fora_hip_sparse_softmax, fora_hip_sparse_softmax_bwd) on the GPU: the softmax inside every held row and its
gradient, bit for bit against the numpy twin of the contract (tests/softmax_ref.py), and exp_def on the device alone
(fora_hip_test_exp).  Every bit-order assertion is made on out64; out32 is checked as (float)out64."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import softmax_ref as sm
from test_sparse_gpu import SEED, _mixed_sources, _raw_fetch

pytestmark = pytest.mark.gpu
ROW_LENS, EMPTY = sm.ROW_LENS, sm.EMPTY
SCALES = [1.0, 0.37, -2.0, 0.0]
QNAN = 0x7FF8000000000000


def _load(engine, g, **kw):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(seed=SEED, epsilon=0.5, **kw)


def _scores(e, dtype, seed):
    """spread over about +-30: exp spans 26 decades inside a row, so the order of the additions shows in the bits"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return ((rng.random(e) * 2 - 1) * 30).astype(dtype)


@pytest.fixture(scope="module")
def held(engine_test, tiny):
    """the held result of the injected rows on the test build's engine, and the twins of the cases -- made once, never changed"""
    _load(engine_test, tiny)
    rows_fix = sm.injected_rows(tiny.n)
    h = {"n": tiny.n, "nq": len(ROW_LENS), "fwd": {}}

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
    engine_test.set_option("softmax_short", 256)


def _fwd_twin(held, dtype, scale):
    key = (np.dtype(dtype).name, scale)
    if key not in held["fwd"]:
        held["fwd"][key] = sm.softmax_ref(held["row_ptr"], _scores(held["entries"], dtype, 9200), scale)
    return held["fwd"][key]


def _same(got64, got32, want64, want32, what):
    assert (got64.view(np.uint64) == want64.view(np.uint64)).all(), what
    assert (got32.view(np.uint32) == want32.view(np.uint32)).all(), what
    assert (got32.view(np.uint32) == got64.astype(np.float32).view(np.uint32)).all(), what


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forward_equals_the_twin(engine_test, tiny, held, dtype):
    _ensure_held(engine_test, tiny, held)
    row_ptr, e = held["row_ptr"], held["entries"]
    scores = _scores(e, dtype, 9200)
    for scale in SCALES:
        want64, want32, nan_rows = _fwd_twin(held, dtype, scale)
        assert nan_rows == 0 and np.isfinite(want64).all()
        o32, o64, st = engine_test.sparse_softmax(row_ptr, scores, scale=scale, want64=True)
        assert o32.shape == o64.shape == (e,)
        _same(o64, o32, want64, want32, (dtype, scale))
        ref = sm.softmax_stats_ref(row_ptr)
        assert {k: st[k] for k in ref} == ref and st["nan_rows"] == 0 and st["in_on_device"] == 0 and st["grad_on_device"] == 0 and st["softmax_ms"] >= 0.0
    # one output at a time, and a caller-made output longer than the entries keeps its tail
    want64, want32, _ = _fwd_twin(held, dtype, 0.37)
    a32, a64, _ = engine_test.sparse_softmax(row_ptr, scores, scale=0.37, want32=True, want64=False)
    b32, b64, _ = engine_test.sparse_softmax(row_ptr, scores, scale=0.37, want32=False, want64=True)
    assert a64 is None and b32 is None
    assert (b64.view(np.uint64) == want64.view(np.uint64)).all() and (a32.view(np.uint32) == want32.view(np.uint32)).all()
    long64 = np.full(e + 4, -77.0, dtype=np.float64)
    engine_test.sparse_softmax(row_ptr, scores, scale=0.37, want32=False, out64=long64)
    assert (long64[:e].view(np.uint64) == want64.view(np.uint64)).all() and (long64[e:] == -77.0).all()


def test_backward_equals_the_twin(engine_test, tiny, held):
    _ensure_held(engine_test, tiny, held)
    row_ptr, e = held["row_ptr"], held["entries"]
    y64, y32, _ = _fwd_twin(held, np.float64, 1.0)
    rng = np.random.Generator(np.random.PCG64(9210))
    g64 = rng.standard_normal(e) * np.exp2(rng.integers(-8, 9, size=e))
    g32 = g64.astype(np.float32)
    for y in (y32, y64):
        for g in (g32, g64):
            for scale in SCALES:
                want64, want32 = sm.softmax_bwd_ref(row_ptr, y, g, scale)
                for short in (256, 0):
                    engine_test.set_option("softmax_short", short)
                    o32, o64, st = engine_test.sparse_softmax_bwd(row_ptr, y, g, scale=scale, want64=True)
                    _same(o64, o32, want64, want32, (y.dtype, g.dtype, scale, short))
                    ref = sm.softmax_stats_ref(row_ptr, short)
                    assert {k: st[k] for k in ref} == ref and st["nan_rows"] == 0
    engine_test.set_option("softmax_short", 256)


def test_options_and_batch_change_no_bit(engine_test, tiny, held):
    _ensure_held(engine_test, tiny, held)
    row_ptr, e = held["row_ptr"], held["entries"]
    scores = _scores(e, np.float32, 9200)
    want64, want32, _ = _fwd_twin(held, np.float32, 0.37)
    g = np.random.Generator(np.random.PCG64(9220)).standard_normal(e).astype(np.float32)
    bwd64, bwd32 = sm.softmax_bwd_ref(row_ptr, want32, g, 0.37)
    try:
        for short, b, segs in ((0, 0, 0), (64, 1, 1), (256, 7, 3), (1, 0, 2), (1000, 3, 0)):
            engine_test.set_option("softmax_short", short)
            engine_test.set_batch(b)
            engine_test.set_option("prop_segs", segs)
            o32, o64, st = engine_test.sparse_softmax(row_ptr, scores, scale=0.37, want64=True)
            _same(o64, o32, want64, want32, (short, b, segs))
            ref = sm.softmax_stats_ref(row_ptr, short)
            assert {k: st[k] for k in ref} == ref, (short, st)
            o32, o64, st = engine_test.sparse_softmax_bwd(row_ptr, want32, g, scale=0.37, want64=True)
            _same(o64, o32, bwd64, bwd32, (short, b, segs))
    finally:
        engine_test.set_batch(0)                     # (the request a fresh context has)
        engine_test.set_option("prop_segs", 0)
        engine_test.set_option("softmax_short", 256)


def test_special_rows(engine_test, tiny, held):
    """NaN rows (a NaN entry, +inf, all -inf) on either path, a single -inf and entries more than 708 below the maximum as
    +0.0, scale = 0, the argmax entry as 1 / S, and the tail of a longer output"""
    _ensure_held(engine_test, tiny, held)
    row_ptr, e = held["row_ptr"], held["entries"]
    row = {L: i for i, L in enumerate(ROW_LENS)}
    scores = _scores(e, np.float64, 9230)
    at = lambda L, j: int(row_ptr[row[L]]) + j
    scores[at(63, 40)] = np.nan                                          # a NaN entry, short path
    scores[at(65, 64)] = np.inf                                          # +inf in the second stride of a lane
    scores[row_ptr[row[2]]:row_ptr[row[2] + 1]] = -np.inf                # every entry -inf
    scores[at(600, 599)] = np.nan                                        # a NaN in the last segment of a long row
    scores[at(257, 256)] = -np.inf                                       # a single -inf, alone in its segment
    scores[at(64, 3)] = -np.inf
    scores[at(255, 7)] = 800.0                                           # everything else in the row is more than 708 below
    scores[at(255, 8)] = 800.0 - 708.0                                   # ... but this one, exactly at the edge
    scores[at(256, 100)] = -0.0
    nan_lens = {63, 65, 2, 600}
    for short in (256, 0, 64):
        engine_test.set_option("softmax_short", short)
        for scale in (1.0, 0.0):
            want64, want32, nan_rows = sm.softmax_ref(row_ptr, scores, scale)
            assert nan_rows == (4 if scale else 6)                       # scale = 0 turns the two rows with a -inf into NaN rows too
            long32, long64 = np.full(e + 3, -9.0, np.float32), np.full(e + 3, -9.0, np.float64)
            _, _, st = engine_test.sparse_softmax(row_ptr, scores, scale=scale, out32=long32, out64=long64)
            _same(long64[:e], long32[:e], want64, want32, (short, scale))
            assert (long32[e:] == -9.0).all() and (long64[e:] == -9.0).all() and st["nan_rows"] == nan_rows
            if scale:
                for i, L in enumerate(ROW_LENS):
                    y = long64[row_ptr[i]:row_ptr[i + 1]]
                    if L in nan_lens:
                        assert (y.view(np.uint64) == QNAN).all() and (long32[row_ptr[i]:row_ptr[i + 1]].view(np.uint32) == 0x7FC00000).all()
                    elif L:
                        assert ((y >= 0.0) & (y <= 1.0)).all()
                        x = scores[row_ptr[i]:row_ptr[i + 1]]
                        S = sm.row_sum(sm.exp_def(x - x.max()))
                        assert y[int(np.argmax(x))].view(np.uint64) == np.float64(1.0 / S).view(np.uint64)
                assert long64[at(257, 256)].view(np.uint64) == 0 and long64[at(64, 3)].view(np.uint64) == 0      # +0.0
                y255 = long64[row_ptr[row[255]]:row_ptr[row[255] + 1]]
                assert y255[7] == 1.0                                    # S = 1 + exp_def(-708) = 1
                assert (np.delete(y255, [7, 8]).view(np.uint64) == 0).all() and y255[8] >= 2.0 ** -1022
    engine_test.set_option("softmax_short", 256)


def _check_held(engine, row_ptr, seed):
    e = int(row_ptr[-1])
    for dtype, scale in ((np.float32, 0.37), (np.float64, -2.0)):
        scores = _scores(e, dtype, seed)
        want64, want32, nan_rows = sm.softmax_ref(row_ptr, scores, scale)
        o32, o64, st = engine.sparse_softmax(row_ptr, scores, scale=scale, want64=True)
        _same(o64, o32, want64, want32, (dtype, scale))
        ref = sm.softmax_stats_ref(row_ptr)
        assert {k: st[k] for k in ref} == ref and st["nan_rows"] == nan_rows == 0
        g = np.random.Generator(np.random.PCG64(seed + 1)).standard_normal(e).astype(dtype)
        b64, b32 = sm.softmax_bwd_ref(row_ptr, want32, g, scale)
        o32, o64, _ = engine.sparse_softmax_bwd(row_ptr, want32, g, scale=scale, want64=True)
        _same(o64, o32, b64, b32, ("bwd", dtype, scale))


def test_real_held_results_equal_the_twin(engine, tiny_dangling):
    """the held result of a query, of a top-k query and of a seed-set call work as the injected rows do"""
    g = tiny_dangling
    srcs = _mixed_sources(g, 9300)                # a duplicate and a dangling source
    _load(engine, g)
    row_ptr, ids, vals, st, sp = engine.query_sparse(srcs, threshold=0.0)
    _check_held(engine, row_ptr, 9300)
    row_ptr, ids, vals, st, sp, tk = engine.query_sparse_topk(srcs, 64, threshold=0.0)
    assert int(np.diff(row_ptr).max()) == 64
    _check_held(engine, row_ptr, 9310)
    live = [int(s) for s in srcs if g.deg[s] > 0]
    r = engine.query_seeds_sparse([live[:3], live[2:5]], [[0.5, 0.25, 0.25], [3.0, 1.0, 2.0]], threshold=1.0 / g.n)
    _check_held(engine, r["row_ptr"], 9320)


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def _raw(engine, row_ptr, nq, s, st, scale, o32, o64, cap):
    return engine._lib.fora_hip_sparse_softmax(engine._ctx, _p(row_ptr), C.c_int(nq), _p(s), C.c_int(st), C.c_double(scale), _p(o32), _p(o64), C.c_uint64(cap), None)


def _raw_bwd(engine, row_ptr, nq, y, yt, g, gt, scale, o32, o64, cap):
    return engine._lib.fora_hip_sparse_softmax_bwd(engine._ctx, _p(row_ptr), C.c_int(nq), _p(y), C.c_int(yt), _p(g), C.c_int(gt), C.c_double(scale),
                                                   _p(o32), _p(o64), C.c_uint64(cap), None)


def test_argument_errors(engine, tiny):
    g = tiny
    _load(engine, g)
    srcs = _mixed_sources(g, 9400)
    nq = len(srcs)
    engine.sparse_clear()
    big = 1 << 20
    s = _scores(big, np.float32, 9401)
    o32, o64 = np.full(big, -5.0, np.float32), np.full(big, -5.0, np.float64)
    assert _raw(engine, np.zeros(nq + 1, np.int64), nq, s, 0, 1.0, o32, o64, big) == -1      # no held result
    assert _raw_bwd(engine, np.zeros(nq + 1, np.int64), nq, s, 0, s, 0, 1.0, o32, o64, big) == -1
    row_ptr, ids, vals, st, sp = engine.query_sparse(srcs, threshold=1.0 / g.n)
    e = sp["entries"]
    assert 0 < e <= big
    end, dec, first, short = row_ptr.copy(), row_ptr.copy(), row_ptr.copy(), row_ptr.copy()
    end[-1] += 1
    dec[2] = dec[1] - 1
    first[0] = 1
    short[-1] -= 1
    for bad in (end, short, dec, first, None):
        assert _raw(engine, bad, nq, s, 0, 1.0, o32, o64, big) == -1                        # a row_ptr that is not the held result's
        assert _raw_bwd(engine, bad, nq, s, 0, s, 0, 1.0, o32, o64, big) == -1
    assert _raw(engine, row_ptr, -1, s, 0, 1.0, o32, o64, big) == -1
    assert _raw(engine, row_ptr, nq, s, 0, 1.0, o32, o64, e - 1) == -1                      # cap too small
    assert _raw(engine, row_ptr, nq, s, 0, 1.0, None, None, big) == -1                      # both outputs NULL
    assert _raw(engine, row_ptr, nq, s, 1, 1.0, o32, o64, big) == -1                        # bf16 is no score type
    assert _raw(engine, row_ptr, nq, s, 3, 1.0, o32, o64, big) == -1
    assert _raw(engine, row_ptr, nq, None, 0, 1.0, o32, o64, big) == -1                     # NULL scores with entries to read
    for bad_scale in (np.nan, np.inf, -np.inf):
        assert _raw(engine, row_ptr, nq, s, 0, bad_scale, o32, o64, big) == -1
        assert _raw_bwd(engine, row_ptr, nq, s, 0, s, 0, bad_scale, o32, o64, big) == -1
    assert _raw_bwd(engine, row_ptr, -1, s, 0, s, 0, 1.0, o32, o64, big) == -1
    assert _raw_bwd(engine, row_ptr, nq, s, 0, s, 0, 1.0, o32, o64, e - 1) == -1
    assert _raw_bwd(engine, row_ptr, nq, s, 0, s, 0, 1.0, None, None, big) == -1
    assert _raw_bwd(engine, row_ptr, nq, s, 1, s, 0, 1.0, o32, o64, big) == -1
    assert _raw_bwd(engine, row_ptr, nq, s, 0, s, 1, 1.0, o32, o64, big) == -1
    assert _raw_bwd(engine, row_ptr, nq, None, 0, s, 0, 1.0, o32, o64, big) == -1
    assert _raw_bwd(engine, row_ptr, nq, s, 0, None, 0, 1.0, o32, o64, big) == -1
    assert (o32 == -5.0).all() and (o64 == -5.0).all()                                      # nothing was written
    i2 = np.zeros(e, np.int32)
    assert _raw_fetch(engine, i2, None, None, e) == 0 and (i2 == ids).all()                  # the held result is intact
    assert _raw(engine, row_ptr, nq, s, 0, 0.37, o32, o64, e) == 0                           # ... and usable
    want64, want32, _ = sm.softmax_ref(row_ptr, s[:e], 0.37)
    _same(o64[:e], o32[:e], want64, want32, "after the errors")
    assert (o32[e:] == -5.0).all() and (o64[e:] == -5.0).all()
    # the binding refuses what the C ABI cannot express
    with pytest.raises(ValueError):
        engine.sparse_softmax(row_ptr, s[:e + 1])
    with pytest.raises(ValueError):
        engine.sparse_softmax(row_ptr, s[:e].astype(np.float16))
    with pytest.raises(ValueError):
        engine.sparse_softmax_bwd(row_ptr, s[:e], s[:e - 1])
    # nq == 0, an empty held result: FORA_OK, nothing written
    engine.query_sparse(np.zeros(0, np.int32))
    o32[:] = -5.0
    assert _raw(engine, np.zeros(1, np.int64), 0, None, 0, 1.0, o32, None, 0) == 0
    assert _raw_bwd(engine, np.zeros(1, np.int64), 0, None, 0, None, 0, 1.0, o32, None, 0) == 0
    assert (o32 == -5.0).all()


def test_exp_def_on_the_device_equals_the_twin(engine_test):
    grid = sm.exp_grid()
    got = engine_test.test_exp(grid)
    want = sm.exp_def(grid)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert bad.size == 0, [(float(grid[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]]
    assert engine_test.test_exp(np.zeros(0)).size == 0


def test_device_operands_and_outputs():
    """scores, y, grad and the outputs as torch tensors on the GPU, in a fresh child process (tests/softmax_device_child.py):
    torch and the library must live on one HIP runtime, so the child imports torch before the library is loaded."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "softmax_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "softmax device ok" in r.stdout
