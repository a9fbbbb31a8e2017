"""Sparse SSPPR results (fora_hip_query_sparse_batch / fora_hip_sparse_fetch / fora_hip_sparse_clear) on the GPU.

The yardstick is the dense result of the same context (fora_hip_query_batch_fix), which the parity tests pin to
oracle/fora_twin.c bit for bit: per row keep = want >= thr_fix, and row_ptr, ids == flatnonzero(keep),
fix == want[keep], vals == ldexp(fix, -62) and the per-query stats must match exactly."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import pick_sources
from growth_case import growth_case, growths_with_entries_to_keep

pytestmark = pytest.mark.gpu
SEED = 0x464F5241
FIX_ONE = 1 << 62
LAYOUTS = {
    "team": {},
    "bucketed": {"team": 0, "tail": 0},
    "wide": {"force_wide": 1},
    "direct": {"direct": 1},
}


def thr_fix_of(t):
    return 1 if t <= 0 else max(1, math.ceil(math.ldexp(t, 62)))


def _load(engine, g, **kw):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(seed=SEED, **kw)
    return engine.get_params()


def _mixed_sources(g, seed):
    """five live sources, a dangling one in the middle (when the graph has one), one live source twice"""
    live = list(pick_sources(g, 5, seed))
    dang = list(pick_sources(g, 1, seed + 1, want_dangling=True))
    return np.array(live[:3] + dang + live[3:] + live[1:2], dtype=np.int32)


def check_against_dense(want, wst, thr, row_ptr, ids, vals, fix, st, sp, batches=None):
    """the whole contract of one sparse call against the dense rows `want` (u64 [nq, n]) and stats `wst` of the same sources"""
    nq = want.shape[0]
    assert row_ptr.dtype == np.int64 and ids.dtype == np.int32 and vals.dtype == np.float64 and fix.dtype == np.uint64
    assert row_ptr.shape == (nq + 1,) and row_ptr[0] == 0
    assert ids.shape == vals.shape == fix.shape == (int(row_ptr[-1]),)
    longest = 0
    for i in range(nq):
        keep = want[i] >= np.uint64(thr)
        lo, hi = int(row_ptr[i]), int(row_ptr[i + 1])
        assert hi - lo == int(keep.sum()), (i, hi - lo, int(keep.sum()))
        assert (ids[lo:hi] == np.flatnonzero(keep)).all(), i
        assert (fix[lo:hi] == want[i][keep]).all(), i
        assert hi - lo <= FIX_ONE // thr
        longest = max(longest, hi - lo)
    assert (vals == np.ldexp(fix.astype(np.float64), -62)).all()
    assert st.dtype == wst.dtype and len(st) == nq
    for name in st.dtype.names:
        assert (st[name] == wst[name]).all(), name
    assert sp["entries"] == int(row_ptr[-1]) and sp["max_row"] == longest and sp["thr_fix"] == thr
    if batches is not None:
        assert sp["batches"] == batches
    assert sp["compact_ms"] >= 0.0


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("gname", ["tiny_dangling", "small"])
def test_sparse_equals_thresholded_dense(engine, oracle, request, gname, layout):
    g = request.getfixturevalue(gname)
    srcs = _mixed_sources(g, 4100)
    ndang = int((g.deg[srcs] == 0).sum())
    assert ndang == (1 if gname == "tiny_dangling" else 0)
    try:
        for name, v in LAYOUTS[layout].items():
            engine.set_option(name, v)
        for opt in (False, True):
            rmax, omega = _load(engine, g, epsilon=0.5, opt=opt)
            for with_idx in (False, True):
                if with_idx:
                    engine.build_index()
                want, _, wst = engine.query_fix(srcs, with_idx=with_idx)
                for t in (0.0, 1.0 / g.n, 1e-3, 0.3, 1.0):
                    thr = thr_fix_of(t)
                    row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, with_idx=with_idx, threshold=t, want_fix=True)
                    check_against_dense(want, wst, thr, row_ptr, ids, vals, fix, st, sp, batches=1)
                    lens = np.diff(row_ptr)
                    if t == 0.0:
                        for i in range(len(srcs)):
                            assert int(fix[row_ptr[i]:row_ptr[i + 1]].sum()) == FIX_ONE == int(st[i]["ppr_sum_fix"])
                    if t == 1.0:
                        for i, s in enumerate(srcs):
                            if g.deg[s] == 0:
                                assert lens[i] == 1 and ids[row_ptr[i]] == s and fix[row_ptr[i]] == FIX_ONE
                            elif want[i][s] < FIX_ONE:
                                assert lens[i] == 0
            if layout == "team" and not opt:   # (the index of the last loop pass is loaded) the twin itself, once per graph
                idx = engine.get_index()
                row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, with_idx=True, threshold=0.0, want_fix=True)
                for i, s in enumerate(srcs):
                    tw, _, _ = oracle.twin_query(g, int(s), rmax, omega, seed=SEED, index=idx)
                    nz = np.flatnonzero(tw)
                    assert (ids[row_ptr[i]:row_ptr[i + 1]] == nz).all() and (fix[row_ptr[i]:row_ptr[i + 1]] == tw[nz]).all()
    finally:
        engine.clear_index()
        engine.reset_options()


def test_several_batches_with_a_dangling_row_between_them(engine, tiny_dangling):
    g = tiny_dangling
    live = list(pick_sources(g, 5, 4200))
    dang = list(pick_sources(g, 2, 4201, want_dangling=True))
    # live slots: rows 0 1 | 3 4 | 5 7 -- row 2 (dangling) falls between the first two batches, row 6 inside the last, row 8 after it
    srcs = np.array(live[:2] + dang[:1] + live[2:5] + dang[1:] + live[:1] + dang[:1], dtype=np.int32)
    _load(engine, g, epsilon=0.5)
    engine.set_batch(2)
    try:
        want, _, wst = engine.query_fix(srcs)
        for t in (0.0, 1.0 / g.n, 1.0):
            row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, threshold=t, want_fix=True)
            check_against_dense(want, wst, thr_fix_of(t), row_ptr, ids, vals, fix, st, sp, batches=3)
        # only dangling sources: no batch at all
        d = np.array(dang + dang[:1], dtype=np.int32)
        row_ptr, ids, vals, fix, st, sp = engine.query_sparse(d, threshold=0.5, want_fix=True)
        assert (row_ptr == np.arange(len(d) + 1)).all() and (ids == d).all() and (fix == FIX_ONE).all() and (vals == 1.0).all()
        assert sp["batches"] == 0 and sp["entries"] == len(d) and sp["max_row"] == 1
        # no source at all
        row_ptr, ids, vals, st, sp = engine.query_sparse(np.zeros(0, dtype=np.int32))
        assert (row_ptr == [0]).all() and ids.size == 0 and vals.size == 0 and sp["entries"] == 0
    finally:
        engine.set_batch(0)


def test_growth_with_entries_to_keep(engine, small):
    """the held arrays grow in the middle of a call and the entries written so far move into the new ones"""
    g, srcs = growth_case(engine, small)
    engine.set_batch(1)
    try:
        want, _, wst = engine.query_fix(srcs)
        lens = (want != 0).sum(axis=1)
        print("row lengths", lens.tolist(), "growths with entries to keep", growths_with_entries_to_keep(lens))
        assert lens[0] == 2 and growths_with_entries_to_keep(lens) >= 2
        engine.sparse_clear()
        row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, threshold=0.0, want_fix=True)
        check_against_dense(want, wst, 1, row_ptr, ids, vals, fix, st, sp, batches=6)
    finally:
        engine.set_batch(0)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 129, 8191, 8192, 8193])
def test_rings(engine, oracle, n):
    """every node one out-edge (n = 1: the edge is a self loop, which the loader drops -- the smallest graph of the edge-case
    tests, a single dangling node): slabs shorter than one wave's range, slab starts at odd words, ranges that end one
    id before / at / after a 16-byte line"""
    import fora_amd
    v = np.arange(n, dtype=np.int32)
    g = oracle.Graph.from_edges(n, max(1, n), v, (v + 1) % n) if n > 1 else \
        oracle.Graph.from_edges(1, 1, np.zeros(0, np.int32), np.zeros(0, np.int32))
    try:
        _load(engine, g, epsilon=0.5)
    except fora_amd.ForaError as e:
        if n == 1 and e.code == -1:
            return   # set_graph / set_params refuse n = 1: the ladder starts at 2
        raise
    srcs = np.array([n - 1, n // 2], dtype=np.int32)
    want, _, wst = engine.query_fix(srcs)
    row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, threshold=0.0, want_fix=True)
    check_against_dense(want, wst, 1, row_ptr, ids, vals, fix, st, sp)
    for i in range(2):
        assert int(fix[row_ptr[i]:row_ptr[i + 1]].sum()) == FIX_ONE


def _raw_fetch(engine, ids, vals, fix, cap):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return engine._lib.fora_hip_sparse_fetch(engine._ctx, p(ids), p(vals), p(fix), C.c_uint64(cap))


def test_lifetime_of_the_held_result(engine, small):
    g = small
    _load(engine, g, epsilon=0.5)
    a = pick_sources(g, 4, 4300)
    b = pick_sources(g, 3, 4301)
    row_ptr, ids, vals, fix, st, sp = engine.query_sparse(a, want_fix=True)
    e = sp["entries"]
    assert e > 0

    def fetched():
        i2, v2, f2 = np.zeros(e, np.int32), np.zeros(e, np.float64), np.zeros(e, np.uint64)
        assert _raw_fetch(engine, i2, v2, f2, e) == 0
        return i2, v2, f2

    # other entry points (and what they do to the workspace) leave it alone
    engine.query_fix(b)
    engine.topk(b, 10)
    engine.fwdpush(b)
    engine.montecarlo(b[:1])
    engine.set_batch(3)
    engine.query(b, want_ppr=False)
    engine.set_batch(0)
    engine.set_option("team", 0)
    engine.query(b, want_ppr=False)
    engine.reset_options()
    for _ in range(2):
        i2, v2, f2 = fetched()
        assert (i2 == ids).all() and (v2 == vals).all() and (f2 == fix).all()
    # any subset of the outputs, a larger cap
    f3 = np.zeros(e + 5, np.uint64)
    assert _raw_fetch(engine, None, None, f3, e + 5) == 0 and (f3[:e] == fix).all() and (f3[e:] == 0).all()
    # cap too small: refused, nothing written
    i4, v4, f4 = np.full(e, -7, np.int32), np.full(e, -7.0), np.full(e, 77, np.uint64)
    assert _raw_fetch(engine, i4, v4, f4, e - 1) == -1
    assert (i4 == -7).all() and (v4 == -7.0).all() and (f4 == 77).all()
    # a second sparse call replaces the first
    row_ptr_b, ids_b, vals_b, fix_b, _, sp_b = engine.query_sparse(b, threshold=1e-3, want_fix=True)
    want_b, _, _ = engine.query_fix(b)
    keep = want_b >= np.uint64(thr_fix_of(1e-3))
    assert sp_b["entries"] == int(keep.sum()) and (fix_b == want_b[keep]).all()
    eb = sp_b["entries"]
    i5 = np.zeros(eb, np.int32)
    assert _raw_fetch(engine, i5, None, None, eb) == 0 and (i5 == ids_b).all()
    # clear: nothing to fetch
    engine.sparse_clear()
    assert _raw_fetch(engine, i4, v4, f4, e) == -1 and (i4 == -7).all()
    engine.sparse_clear()   # (twice is fine)
    # set_graph drops the result
    engine.query_sparse(a)
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    assert _raw_fetch(engine, i4, v4, f4, e) == -1 and (i4 == -7).all() and (f4 == 77).all()
    engine.set_params(epsilon=0.5, seed=SEED)
    # ... and the first call after it gives the same rows again
    r2, i6, v6, f6, _, _ = engine.query_sparse(a, want_fix=True)
    assert (r2 == row_ptr).all() and (i6 == ids).all() and (f6 == fix).all()


def test_device_fetch_and_torch_csr():
    """query_sparse(device=True) and to_torch_csr, in a child of their own (tests/sparse_device_child.py): torch tensors
    and the library must live on one HIP runtime, so the child imports torch before the library is loaded -- this
    process loaded the library first (the `engine` fixture), and a torch imported now would bring a second runtime."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "sparse_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "sparse device ok" in r.stdout


def test_sparse_call_disturbs_nothing(engine, small):
    g = small
    _load(engine, g, epsilon=0.5)
    srcs = _mixed_sources(g, 4500)
    ppr0, res0, st0 = engine.query_fix(srcs)
    params, batch = engine.get_params(), engine.get_batch()   # (the slots of the workspace the first call planned)
    engine.reset_timing()
    engine.query(srcs, want_ppr=False)
    td = engine.timing()
    engine.reset_timing()
    engine.query_sparse(srcs)
    ts = engine.timing()
    for k in ("batches", "pops", "relax", "walks"):
        assert ts[k] == td[k] and td[k] > 0, k
    ppr1, res1, st1 = engine.query_fix(srcs)
    assert (ppr1 == ppr0).all() and (res1 == res0).all()
    for name in st0.dtype.names:
        assert (st1[name] == st0[name]).all()
    assert engine.get_params() == params and engine.get_batch() == batch


def test_argument_errors(engine, small):
    import fora_amd
    g = small
    _load(engine, g, epsilon=0.5)
    ok = pick_sources(g, 2, 4600)
    lib, ctx = engine._lib, engine._ctx
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(src, nq, with_idx, t, row_ptr):
        return lib.fora_hip_query_sparse_batch(ctx, p(src), C.c_int(nq), C.c_int(with_idx), C.c_double(t),
                                               p(row_ptr) if row_ptr is not None else None, None, None)

    rp = np.zeros(3, np.int64)
    assert call(ok, 2, 0, 0.0, rp) == 0                     # a held result ...
    assert call(np.array([0, g.n], np.int32), 2, 0, 0.0, rp) == -1
    assert call(np.array([-1, 0], np.int32), 2, 0, 0.0, rp) == -1
    assert call(ok, -1, 0, 0.0, rp) == -1
    assert call(ok, 2, 0, 1.5, rp) == -1
    assert call(ok, 2, 0, float("nan"), rp) == -1
    assert call(ok, 2, 0, 0.0, None) == -1
    assert call(ok, 2, 1, 0.0, rp) == -1                    # no index
    buf = np.zeros(g.n * 2, np.int32)
    assert _raw_fetch(engine, buf, None, None, buf.size) == -1   # ... does not outlive a failed call
    with pytest.raises(fora_amd.ForaError) as ei:
        engine.query_sparse(ok, threshold=2.0)
    assert ei.value.code == -1
    _, st = engine.query(ok, want_ppr=False)
    assert all(int(s["ppr_sum_fix"]) == FIX_ONE for s in st)
    row_ptr, ids, vals, st, sp = engine.query_sparse(ok, threshold=0.0)
    assert sp["entries"] == ids.size > 0 and abs(vals.sum() - 2.0) < 1e-9


def test_bucket_retry_leaves_no_rows_behind(engine, small):
    """message buckets far too small: the sparse call is run again with doubled buckets until the push fits (as its dense
    siblings are); the rows are those of the attempt that went through"""
    g = small
    engine.set_option("team", 0)
    engine.set_option("bkcap", 8)
    engine.set_option("ovcap", 64)
    engine.set_option("tail", 0)
    try:
        _load(engine, g, epsilon=0.5)
        srcs = pick_sources(g, 4, 4700)
        r0 = engine.get_option("bucket_retries")
        row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, threshold=0.0, want_fix=True)
        assert engine.get_option("bucket_retries") > r0
        want, _, wst = engine.query_fix(srcs)
        check_against_dense(want, wst, 1, row_ptr, ids, vals, fix, st, sp, batches=1)
    finally:
        engine.reset_options()
        engine.set_graph(g.n, g.m, g.row_ptr, g.col)   # a new graph starts from the default capacity again


def _row_invariants(row_ptr, ids, vals, fix, st, sp, thr, n):
    nq = len(row_ptr) - 1
    lens = np.diff(row_ptr)
    assert row_ptr[0] == 0 and (lens >= 0).all() and int(row_ptr[-1]) == sp["entries"] == ids.size == fix.size == vals.size
    assert int(lens.max()) == sp["max_row"] and sp["max_row"] <= FIX_ONE // thr and sp["thr_fix"] == thr
    assert (fix >= np.uint64(thr)).all() and (ids >= 0).all() and (ids < n).all()
    assert (vals == np.ldexp(fix.astype(np.float64), -62)).all()
    starts = np.zeros(ids.size, dtype=bool)
    starts[row_ptr[:-1][lens > 0]] = True
    assert (np.diff(ids.astype(np.int64))[~starts[1:]] > 0).all()      # ids ascend inside every row
    sums = np.add.reduceat(fix, row_ptr[:-1][lens > 0]) if ids.size else np.zeros(0, np.uint64)
    assert (sums <= np.uint64(FIX_ONE)).all()
    assert all(int(s["ppr_sum_fix"]) == FIX_ONE for s in st) and len(st) == nq


def test_webstanford_sized_three_batches(engine):
    from fora_amd import synth
    n, m, row_ptr_g, col = synth.preset("webstanford")
    engine.clear_index()
    engine.set_graph(n, m, row_ptr_g, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    srcs = synth.query_set(n, 300, 11)
    thr = thr_fix_of(1.0 / n)
    engine.set_batch(100)
    try:
        row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, want_fix=True)     # threshold None: 1 / n
        assert sp["batches"] == 3
        print("webstanford-sized: entries per row mean %.1f max %d, compact_ms %.3f" % (sp["entries"] / 300.0, sp["max_row"], sp["compact_ms"]))
        _row_invariants(row_ptr, ids, vals, fix, st, sp, thr, n)
    finally:
        engine.set_batch(0)
    pick = np.arange(0, 300, 19)[:16]                                                  # rows of all three batches
    want, _, wst = engine.query_fix(srcs[pick])
    for j, i in enumerate(pick):
        keep = want[j] >= np.uint64(thr)
        lo, hi = int(row_ptr[i]), int(row_ptr[i + 1])
        assert hi - lo == int(keep.sum())
        assert (ids[lo:hi] == np.flatnonzero(keep)).all() and (fix[lo:hi] == want[j][keep]).all()
        for name in st.dtype.names:
            assert st[i][name] == wst[j][name], name


def test_medium_wide_graph(engine):
    """n >= 2^20 (1.5 M nodes, the wide layout; built as the `medium` fixture of test_large_gpu.py builds it)"""
    from fora_amd import synth
    n, m, row_ptr_g, col = synth.preset("medium")
    assert n >= 1 << 20
    engine.clear_index()
    engine.set_graph(n, m, row_ptr_g, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    srcs = synth.query_set(n, 4, 13)
    want, _, wst = engine.query_fix(srcs, want_residue=False)
    for t in (0.0, 1.0 / n):
        row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, threshold=t, want_fix=True)
        check_against_dense(want, wst, thr_fix_of(t), row_ptr, ids, vals, fix, st, sp)
