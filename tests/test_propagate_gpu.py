"""PROPAGATE (fora_hip_sparse_propagate) on the GPU: the held sparse rows times a feature matrix, bit for bit against the
numpy twin of the contract (tests/propagate_ref.py).  Every bit-order assertion is made on out64 (tests/test_propagate_cpu.py
shows that float32 outputs cannot tell one order of additions from another); out32 is checked as (float)out64."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import propagate_ref as pr
from test_sparse_gpu import SEED, _mixed_sources, _raw_fetch, thr_fix_of

pytestmark = pytest.mark.gpu
FIX_ONE = 1 << 62
LENS = [0, 1, 2, 255, 256, 257, 511, 512, 513, 1000, None]   # None: n, every node


def _load(engine, g, **kw):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(seed=SEED, epsilon=0.5, **kw)


def injected_rows(n, seed=6100):
    """[len(LENS), n] words: row i has exactly LENS[i] non-zero entries, random in [1, 2^62 / len]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = [n if L is None else L for L in LENS]
    rows = np.zeros((len(lens), n), dtype=np.uint64)
    for i, L in enumerate(lens):
        at = rng.choice(n, size=L, replace=False)
        rows[i, at] = rng.integers(1, FIX_ONE // max(L, 1) + 1, size=L, dtype=np.uint64)
    return rows, lens


@pytest.fixture(scope="module")
def injected(engine_test, tiny):
    """the held result of the injected rows on the test build's engine, and its fetched arrays -- made once, never changed"""
    _load(engine_test, tiny)
    rows, lens = injected_rows(tiny.n)
    held = {"n": tiny.n, "rows": rows, "lens": lens}

    def hold():
        row_ptr, sp = engine_test.test_sparse_rows(rows, threshold=0.0)
        assert np.diff(row_ptr).tolist() == lens and sp["entries"] == sum(lens) and sp["max_row"] == tiny.n
        e = int(row_ptr[-1])
        ids, fix = np.zeros(e, np.int32), np.zeros(e, np.uint64)
        assert _raw_fetch(engine_test, ids, None, fix, e) == 0
        for i in range(len(lens)):
            nz = np.flatnonzero(rows[i])
            assert (ids[row_ptr[i]:row_ptr[i + 1]] == nz).all() and (fix[row_ptr[i]:row_ptr[i + 1]] == rows[i][nz]).all()
        held.update(row_ptr=row_ptr, ids=ids, fix=fix)
    held["hold"] = hold
    hold()
    return held


def _ensure_held(engine_test, tiny, injected):
    """another module may have used the session's test engine in between: put graph and rows back if so"""
    e = int(injected["row_ptr"][-1])
    ids = np.zeros(e, np.int32)
    if engine_test.n != tiny.n or _raw_fetch(engine_test, ids, None, None, e) != 0 or not (ids == injected["ids"]).all():
        _load(engine_test, tiny)
        injected["hold"]()


def _features(n, d, ldf, bf16, seed):
    """[n, d] features as a view of an [n, ldf] array (the padding holds NaN patterns that must never be read into a sum)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    H = pr.scaled_features(rng, n, d)
    if bf16:
        wide = np.full((n, ldf), 0x7FC1, dtype=np.uint16)
        wide[:, :d] = pr.to_bf16_bits(H)
    else:
        wide = np.full((n, ldf), np.nan, dtype=np.float32)
        wide[:, :d] = H
    return wide[:, :d]


def _outputs(nq, d, ldo):
    o32 = np.full((nq, ldo), -77.0, dtype=np.float32)
    o64 = np.full((nq, ldo), -77.0, dtype=np.float64)
    return o32, o64


@pytest.mark.parametrize("d", [1, 2, 3, 16, 63, 64, 65, 128, 130])
def test_injected_rows_equal_the_twin(engine_test, tiny, injected, d):
    _ensure_held(engine_test, tiny, injected)
    n, row_ptr, ids, fix = injected["n"], injected["row_ptr"], injected["ids"], injected["fix"]
    nq = len(row_ptr) - 1
    for bf16 in (False, True):
        elt = 2 if bf16 else 4
        twins = {}
        for ldf in (d, d + 1, d + 3):
            H = _features(n, d, ldf, bf16, 6200 + d)      # the same values at every pitch
            assert H.strides[0] == ldf * elt
            for normalize in (False, True):
                if normalize not in twins:
                    twins[normalize] = pr.propagate_ref(row_ptr, ids, fix, H, normalize=normalize, bf16=bf16)
                want64, want32 = twins[normalize]
                for ldo in (d, d + 5):
                    o32, o64 = _outputs(nq, d, ldo)
                    r32, r64, ps = engine_test.sparse_propagate(row_ptr, H, normalize=normalize, bf16=bf16, out32=o32[:, :d], out64=o64[:, :d])
                    what = (d, bf16, ldf, normalize, ldo)
                    assert (o64[:, :d].view(np.uint64) == want64.view(np.uint64)).all(), what
                    assert (o32[:, :d].view(np.uint32) == want32.view(np.uint32)).all(), what
                    assert (o32[:, :d].view(np.uint32) == o64[:, :d].astype(np.float32).view(np.uint32)).all(), what
                    assert (o32[:, d:] == -77.0).all() and (o64[:, d:] == -77.0).all(), what    # the padding survives
                    ref = pr.prop_stats_ref(row_ptr, d, elt)
                    assert {k: ps[k] for k in ref} == ref and ps["feat_on_device"] == 0 and ps["chunks"] >= 1, what
                    assert ps["gather_ms"] >= 0.0 and ps["combine_ms"] >= 0.0
        # one output at a time
        H = _features(n, d, d, bf16, 6200 + d)
        a32, a64, _ = engine_test.sparse_propagate(row_ptr, H, bf16=bf16, want32=True, want64=False)
        b32, b64, _ = engine_test.sparse_propagate(row_ptr, H, bf16=bf16, want32=False, want64=True)
        assert a64 is None and b32 is None
        assert (b64.view(np.uint64) == twins[False][0].view(np.uint64)).all() and (a32.view(np.uint32) == twins[False][1].view(np.uint32)).all()
    assert (twins[False][0][0] == 0.0).all() and not np.signbit(twins[False][0][0]).any()


def test_prop_segs_changes_no_bit(engine_test, tiny, injected):
    _ensure_held(engine_test, tiny, injected)
    n, row_ptr, ids, fix = injected["n"], injected["row_ptr"], injected["ids"], injected["fix"]
    d = 20
    H = _features(n, d, d, False, 6300)
    segments = pr.prop_stats_ref(row_ptr, d, 4)["segments"]
    assert segments > 3
    try:
        for normalize in (False, True):
            want64, want32 = pr.propagate_ref(row_ptr, ids, fix, H, normalize=normalize)
            for segs, chunks in ((1, segments), (3, -(-segments // 3)), (0, 1), (segments, 1), (segments - 1, 2)):
                engine_test.set_option("prop_segs", segs)
                assert engine_test.get_option("prop_segs") == segs
                o32, o64, ps = engine_test.sparse_propagate(row_ptr, H, normalize=normalize, want64=True)
                assert ps["chunks"] == chunks and ps["segments"] == segments, (segs, ps)
                assert (o64.view(np.uint64) == want64.view(np.uint64)).all(), (segs, normalize)
                assert (o32.view(np.uint32) == want32.view(np.uint32)).all(), (segs, normalize)
    finally:
        engine_test.set_option("prop_segs", 0)


def _check_held(engine, row_ptr, ids, fix, n, seed, cases):
    """sparse_propagate on the held result against the twin fed with the fetched (ids, fix)"""
    for d, bf16, normalize in cases:
        H = _features(n, d, d + (1 if d % 2 else 0), bf16, seed + d)
        want64, want32 = pr.propagate_ref(row_ptr, ids, fix, H, normalize=normalize, bf16=bf16)
        o32, o64, ps = engine.sparse_propagate(row_ptr, H, normalize=normalize, bf16=bf16, want64=True)
        assert (o64.view(np.uint64) == want64.view(np.uint64)).all(), (d, bf16, normalize)
        assert (o32.view(np.uint32) == want32.view(np.uint32)).all(), (d, bf16, normalize)
        ref = pr.prop_stats_ref(row_ptr, d, 2 if bf16 else 4)
        assert {k: ps[k] for k in ref} == ref


@pytest.mark.parametrize("gname", ["tiny_dangling", "small"])
def test_real_rows_equal_the_twin(engine, request, gname):
    g = request.getfixturevalue(gname)
    srcs = _mixed_sources(g, 6400)                # a duplicate, and on tiny_dangling a dangling source
    assert int((g.deg[srcs] == 0).sum()) == (1 if gname == "tiny_dangling" else 0)
    _load(engine, g)
    try:
        for with_idx in (False, True):
            if with_idx:
                engine.build_index()
            for t, cases in ((0.0, [(33, False, False)]), (1.0 / g.n, [(8, True, True)]), (1e-3, [(3, False, True), (64, True, False)])):
                row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, with_idx=with_idx, threshold=t, want_fix=True)
                assert sp["thr_fix"] == thr_fix_of(t)
                _check_held(engine, row_ptr, ids, fix, g.n, 6400, cases)
        # seed sets: a weighted and a uniform one
        live = [int(s) for s in srcs if g.deg[s] > 0]
        sets = [live[:3], live[2:5], [int(srcs[3])] + live[:1]]
        for weights in (None, [[0.5, 0.25, 0.25], [3.0, 1.0, 2.0], [1.0, 7.0]]):
            r = engine.query_seeds_sparse(sets, weights, threshold=1.0 / g.n, want_fix=True)
            _check_held(engine, r["row_ptr"], r["ids"], r["fix"], g.n, 6450, [(17, False, True), (4, True, False)])
        # the conveniences: chunks of sources / sets smaller than the call give the one-call result
        H = _features(g.n, 12, 12, False, 6460)
        one = engine.propagate(srcs, H, threshold=1e-3, want64=True, normalize=True)
        row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, threshold=1e-3, want_fix=True)
        want64, want32 = pr.propagate_ref(row_ptr, ids, fix, H, normalize=True)
        assert (one["out64"].view(np.uint64) == want64.view(np.uint64)).all() and (one["out32"].view(np.uint32) == want32.view(np.uint32)).all()
        assert len(one["prop"]) == 1 and len(one["stats"]) == len(srcs)
        for chunk in (1, 3):
            part = engine.propagate(srcs, H, threshold=1e-3, want64=True, normalize=True, chunk=chunk)
            assert (part["out64"].view(np.uint64) == want64.view(np.uint64)).all() and (part["out32"].view(np.uint32) == want32.view(np.uint32)).all()
            assert len(part["prop"]) == -(-len(srcs) // chunk)
            for name in st.dtype.names:
                assert (part["stats"][name] == st[name]).all(), name
        w = [[0.5, 0.25, 0.25], [3.0, 1.0, 2.0], [1.0, 7.0]]
        one = engine.propagate_seeds(sets, w, H, want64=True)
        r = engine.query_seeds_sparse(sets, w, want_fix=True)
        want64, _ = pr.propagate_ref(r["row_ptr"], r["ids"], r["fix"], H)
        assert (one["out64"].view(np.uint64) == want64.view(np.uint64)).all()
        part = engine.propagate_seeds(sets, w, H, want64=True, chunk=2)
        assert (part["out64"].view(np.uint64) == want64.view(np.uint64)).all() and len(part["prop"]) == 2
    finally:
        engine.clear_index()


@pytest.mark.parametrize("gname", ["tiny_dangling", "small"])
def test_one_hot_columns_give_the_dense_words(engine, request, gname):
    """a yardstick that is not the twin: with H the one-hot columns of 64 nodes, out64[i][c] is exactly the dense row's
    word at that node times 2^-62 where it passes the threshold, and 0.0 elsewhere -- every other term is an exact zero"""
    g = request.getfixturevalue(gname)
    _load(engine, g)
    srcs = _mixed_sources(g, 6500)
    dense, _, _ = engine.query_fix(srcs, want_residue=False)
    rng = np.random.Generator(np.random.PCG64(6501))
    hit = np.argsort(-dense.sum(axis=0, dtype=np.float64))[:48]                       # nodes the rows do reach, and any 16 others
    nodes = np.concatenate([hit, rng.choice(np.setdiff1d(np.arange(g.n), hit), 16, replace=False)])
    H = np.zeros((g.n, 64), dtype=np.float32)
    H[nodes, np.arange(64)] = 1.0
    for t in (0.0, 1.0 / g.n, 1e-3):
        thr = np.uint64(thr_fix_of(t))
        row_ptr, ids, vals, st, sp = engine.query_sparse(srcs, threshold=t)
        o32, o64, _ = engine.sparse_propagate(row_ptr, H, want64=True)
        words = dense[:, nodes]
        want = np.where(words >= thr, np.ldexp(words.astype(np.float64), -62), 0.0)
        assert (o64.view(np.uint64) == want.view(np.uint64)).all()
        assert (want > 0).sum() >= 48 and (o32 == want.astype(np.float32)).all()


def test_state_is_left_alone(engine, small):
    g = small
    _load(engine, g)
    srcs = _mixed_sources(g, 6600)
    sw = engine.sweep(srcs[:3], want_profile=True)
    row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, want_fix=True)
    params, batch = engine.get_params(), engine.get_batch()
    e = sp["entries"]
    engine.reset_timing()
    t0 = engine.timing()
    Ha, Hb = _features(g.n, 10, 10, False, 6601), _features(g.n, 10, 10, False, 6602)
    for H in (Ha, Hb, Ha):                        # two feature matrices on one held result, and the first again
        want64, _ = pr.propagate_ref(row_ptr, ids, fix, H)
        _, o64, _ = engine.sparse_propagate(row_ptr, H, want32=False, want64=True)
        assert (o64.view(np.uint64) == want64.view(np.uint64)).all()
        i2, v2, f2 = np.zeros(e, np.int32), np.zeros(e, np.float64), np.zeros(e, np.uint64)
        assert _raw_fetch(engine, i2, v2, f2, e) == 0
        assert (i2 == ids).all() and (v2 == vals).all() and (f2 == fix).all()
    assert engine.timing() == t0 and engine.get_params() == params and engine.get_batch() == batch
    ids_s, cut_s, vol_s = engine.sweep_fetch(int(sw["row_ptr"][-1]))                  # the held sweep profile survives
    assert (ids_s == sw["ids"]).all() and (cut_s == sw["cut"]).all() and (vol_s == sw["vol"]).all()


def _raw(engine, row_ptr, nq, feat, ftype, d, ldf, flags, out32, out64, ldo):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return engine._lib.fora_hip_sparse_propagate(engine._ctx, p(row_ptr), C.c_int(nq), p(feat), C.c_int(ftype), C.c_int(d), C.c_int64(ldf),
                                                 C.c_int(flags), p(out32), p(out64), C.c_int64(ldo), None)


def test_argument_errors(engine, tiny):
    g = tiny
    _load(engine, g)
    srcs = _mixed_sources(g, 6700)
    d = 6
    H = _features(g.n, d, d, False, 6701)
    nq = len(srcs)
    o32, o64 = np.full((nq, d), -5.0, np.float32), np.full((nq, d), -5.0, np.float64)
    engine.sparse_clear()
    rp0 = np.zeros(nq + 1, np.int64)
    assert _raw(engine, rp0, nq, H, 0, d, d, 0, o32, o64, d) == -1                    # no held result
    row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, want_fix=True)
    engine.sparse_clear()
    assert _raw(engine, row_ptr, nq, H, 0, d, d, 0, o32, o64, d) == -1                # after sparse_clear
    row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, want_fix=True)
    e = sp["entries"]
    end, dec, first = row_ptr.copy(), row_ptr.copy(), row_ptr.copy()
    end[-1] += 1
    dec[2] = dec[1] - 1
    first[0] = 1
    short = row_ptr.copy()
    short[-1] -= 1
    for bad in (end, short, dec, first):
        assert _raw(engine, bad, nq, H, 0, d, d, 0, o32, o64, d) == -1
    assert _raw(engine, None, nq, H, 0, d, d, 0, o32, o64, d) == -1
    assert _raw(engine, row_ptr, -1, H, 0, d, d, 0, o32, o64, d) == -1
    assert _raw(engine, row_ptr, nq, None, 0, d, d, 0, o32, o64, d) == -1             # NULL feat with entries to read
    assert _raw(engine, row_ptr, nq, H, 0, d, d - 1, 0, o32, o64, d) == -1            # ldf < d
    assert _raw(engine, row_ptr, nq, H, 0, d, d, 0, o32, o64, d - 1) == -1            # ldo < d
    assert _raw(engine, row_ptr, nq, H, 0, 0, d, 0, o32, o64, d) == -1                # d = 0
    assert _raw(engine, row_ptr, nq, H, 0, 65537, 65537, 0, o32, o64, 65537) == -1
    assert _raw(engine, row_ptr, nq, H, 0, d, d, 0, None, None, d) == -1              # both outputs NULL
    assert _raw(engine, row_ptr, nq, H, 2, d, d, 0, o32, o64, d) == -1                # a bad feat_type
    assert _raw(engine, row_ptr, nq, H, -1, d, d, 0, o32, o64, d) == -1
    assert _raw(engine, row_ptr, nq, H, 0, d, d, 2, o32, o64, d) == -1                # an unknown flag bit
    assert (o32 == -5.0).all() and (o64 == -5.0).all()                                # nothing was written
    i2, f2 = np.zeros(e, np.int32), np.zeros(e, np.uint64)
    assert _raw_fetch(engine, i2, None, f2, e) == 0 and (i2 == ids).all() and (f2 == fix).all()   # the held result is intact
    assert _raw(engine, row_ptr, nq, H, 0, d, d, 0, o32, o64, d) == 0                 # ... and usable
    want64, want32 = pr.propagate_ref(row_ptr, ids, fix, H)
    assert (o64.view(np.uint64) == want64.view(np.uint64)).all() and (o32.view(np.uint32) == want32.view(np.uint32)).all()
    # the binding refuses what the C ABI cannot express
    with pytest.raises(ValueError):
        engine.sparse_propagate(row_ptr, np.zeros((g.n, 2 * d), np.float32)[:, ::2])  # a column stride of two elements
    with pytest.raises(ValueError):
        engine.sparse_propagate(row_ptr, np.zeros((g.n, d), np.float64))
    # nq == 0: nothing to do, nothing written
    engine.query_sparse(np.zeros(0, np.int32))
    o32[:] = -5.0
    assert _raw(engine, np.zeros(1, np.int64), 0, None, 0, d, d, 0, o32, None, d) == 0 and (o32 == -5.0).all()


def test_device_pointers():
    """feat and the outputs as torch tensors on the GPU (float32 and bfloat16, contiguous and as a column slice of a wider
    tensor), in a fresh child process (tests/propagate_device_child.py): torch and the library must live on one HIP
    runtime, so the child imports torch before the library is loaded."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "propagate_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "propagate device ok" in r.stdout
