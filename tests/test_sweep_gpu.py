"""Local clustering on the GPU (fora_hip_sweep_batch / fora_hip_sweep_fetch / fora_hip_sweep_clear).

The yardstick is tests/sweep_ref.py -- the SWEEP CUT contract in Python ints -- applied to the dense rows of the same context
(fora_hip_query_batch_fix), which the parity tests pin to oracle/fora_twin.c bit for bit.  Everything is asserted equal:
row_ptr, the rows (len, best, cut, vol, den, conductance bit for bit), the fetched order / cut / vol, the per-query stats
field by field, and the entries / max_row / thr_fix of the sweep's stats."""
import ctypes as C
import math

import numpy as np
import pytest

import sweep_ref as R
from conftest import pick_sources
from growth_case import growth_case, growths_with_entries_to_keep

pytestmark = pytest.mark.gpu
SEED = 0x464F5241
FIX_ONE = 1 << 62
THRESHOLDS = (0.0, None, 1e-3, 0.3, 1.0)   # None: 1 / n


class G:
    """a CSR as the engine takes it"""
    def __init__(self, n, row_ptr, col):
        self.n, self.m = int(n), int(row_ptr[-1])
        self.row_ptr, self.col = np.ascontiguousarray(row_ptr, dtype=np.int64), np.ascontiguousarray(col, dtype=np.int32)
        self.deg = np.diff(self.row_ptr)


@pytest.fixture(scope="module")
def planted():
    n, row_ptr, col, block = R.planted_graph()
    g = G(n, row_ptr, col)
    g.block = block
    return g


@pytest.fixture(scope="module")
def star():
    """node 0 has 1500 out-edges (more than a workgroup has lanes), node 1 has 100 (a wave's share), every leaf points back
    at 0, and a ring runs over the nodes 1 .. n - 1"""
    n = 1999
    src = [0] * 1500 + list(range(1, 1501)) + [1] * 100 + list(range(1, n))
    dst = list(range(1, 1501)) + [0] * 1500 + list(range(1501, 1601)) + [i + 1 if i + 1 < n else 1 for i in range(1, n)]
    e = sorted(set(zip(src, dst)))
    src, dst = np.array([a for a, _ in e]), np.array([b for _, b in e], dtype=np.int32)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=row_ptr[1:])
    g = G(n, row_ptr, dst)
    assert g.deg[0] == 1500 and 64 <= g.deg[1] < 256
    return g


@pytest.fixture(scope="module")
def dupes():
    """150 nodes, stored duplicate edges, dangling nodes: straight into set_graph"""
    rng = np.random.Generator(np.random.PCG64(8100))
    n = 150
    deg = rng.integers(1, 7, size=n)
    deg[rng.choice(n, size=20, replace=False)] = 0
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=row_ptr[1:])
    col = np.zeros(int(row_ptr[-1]), dtype=np.int32)
    for u in range(n):
        t = rng.integers(0, n - 1, size=deg[u])
        t = t + (t >= u)
        if deg[u] >= 2:
            t[1] = t[0]
        col[row_ptr[u]:row_ptr[u + 1]] = np.sort(t)
    return G(n, row_ptr, col)


def _load(engine, g, **kw):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(seed=SEED, **kw)


def _mixed_sources(g, seed):
    """five live sources, a dangling one in the middle (when the graph has one), one live source twice"""
    live = list(pick_sources(g, 5, seed))
    dang = list(pick_sources(g, 1, seed + 1, want_dangling=True))
    return np.array(live[:3] + dang + live[3:] + live[1:2], dtype=np.int32)


_MEMO = {}


def _ref(g, row, thr, max_size):
    """the twin of one row, computed once per (graph, row, threshold, max_size)"""
    key = (id(g), hash(row.tobytes()), thr, max_size)
    full = _MEMO.get(key[:3] + (0,))
    if max_size > 0 and full is not None and full["len"] <= max_size:
        return full   # (nothing is cut off: the uncut profile, already computed)
    if key not in _MEMO:
        _MEMO[key] = R.sweep_row(row, g.row_ptr, g.col, thr, max_size)
    return _MEMO[key]


def check(g, want, wst, t, max_size, out):
    """one sweep call `out` (with its profile) against the dense rows `want` and stats `wst` of the same sources (wst None: a
    call over injected rows, tests/test_sweep_shapes_gpu.py -- there are no query stats to compare)"""
    thr = R.thr_fix_of(1.0 / g.n if t is None else t)
    nq = want.shape[0]
    row_ptr, rows, ids, cut, vol = out["row_ptr"], out["rows"], out["ids"], out["cut"], out["vol"]
    assert row_ptr.dtype == np.int64 and row_ptr.shape == (nq + 1,) and row_ptr[0] == 0
    assert ids.dtype == np.int32 and cut.dtype == np.uint64 and vol.dtype == np.uint64
    assert ids.shape == cut.shape == vol.shape == (int(row_ptr[-1]),)
    entries = longest = 0
    for i in range(nq):
        r = _ref(g, want[i], thr, max_size)
        lo, hi = int(row_ptr[i]), int(row_ptr[i + 1])
        assert hi - lo == len(r["order"]), (i, hi - lo, len(r["order"]))
        assert ids[lo:hi].tolist() == r["order"], i
        assert cut[lo:hi].tolist() == r["cut"], i
        assert vol[lo:hi].tolist() == r["vol"], i
        got = rows[i]
        assert (int(got["len"]), int(got["best"]), int(got["cut"]), int(got["vol"]), int(got["den"])) == \
               (r["len"], r["best"], r["cut_best"], r["vol_best"], r["den"]), i
        assert R.f64_bits(got["conductance"]) == R.f64_bits(r["conductance"]), i
        entries += r["len"]
        longest = max(longest, r["len"])
    if wst is not None:
        st = out["stats"]
        assert st.dtype == wst.dtype and len(st) == nq
        for name in st.dtype.names:
            assert (st[name] == wst[name]).all(), name
    sw = out["sweep"]
    assert sw["entries"] == entries and sw["max_row"] == longest and sw["thr_fix"] == thr
    assert sw["compact_ms"] >= 0.0 and sw["sort_ms"] >= 0.0 and sw["cut_ms"] >= 0.0


def _bits(out):
    return (out["row_ptr"].tobytes(), out["rows"].tobytes(), out["ids"].tobytes(), out["cut"].tobytes(), out["vol"].tobytes())


@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling", "planted"])
def test_sweep_equals_twin(engine, request, gname):
    g = request.getfixturevalue(gname)
    srcs = _mixed_sources(g, 8200)
    assert int((g.deg[srcs] == 0).sum()) == (1 if gname == "tiny_dangling" else 0)
    lens = {}
    try:
        for opt in (False, True):
            _load(engine, g, epsilon=0.5, opt=opt)
            for with_idx in (False, True):
                if with_idx:
                    engine.build_index()
                want, _, wst = engine.query_fix(srcs, with_idx=with_idx)
                for t in THRESHOLDS:
                    out = engine.sweep(srcs, with_idx=with_idx, threshold=t, want_profile=True)
                    check(g, want, wst, t, 0, out)
                    lens[t] = out["rows"]["len"]
                    for i, s in enumerate(srcs):
                        if g.deg[s] == 0:
                            assert out["rows"][i]["len"] == 1 and out["ids"][out["row_ptr"][i]] == s and out["rows"][i]["best"] == 0
        live = g.deg[srcs] > 0
        assert (lens[0.0][live] > lens[None][live]).all() and (lens[None][live] > lens[1e-3][live]).all() and (lens[1e-3][live] > 0).all()
        assert (lens[0.3][live] <= 3).all() and (lens[1.0][live] == 0).all()
    finally:
        engine.clear_index()
    if gname == "planted":   # the best clusters, by the public call
        s = g.block[:2]
        want, _, _ = engine.query_fix(s)
        for i, members in enumerate(engine.local_cluster(s)):
            r = _ref(g, want[i], R.thr_fix_of(1.0 / g.n), 0)
            assert members.dtype == np.int32 and members.tolist() == r["order"][:r["best"]] and r["best"] > 0


def test_growth_with_entries_to_keep(engine, small):
    """the held arrays grow in the middle of a call and the profiles written so far move into the new ones (the case of
    growth_case.py: one row per batch, a row of 2 entries and then five long ones)"""
    g, srcs = growth_case(engine, small)
    engine.set_batch(1)
    try:
        want, _, wst = engine.query_fix(srcs)
        lens = (want != 0).sum(axis=1)
        print("row lengths", lens.tolist(), "growths with entries to keep", growths_with_entries_to_keep(lens))
        assert lens[0] == 2 and growths_with_entries_to_keep(lens) >= 2
        engine.sweep_clear()
        out = engine.sweep(srcs, threshold=0.0, want_profile=True)
        check(g, want, wst, 0.0, 0, out)
        assert out["sweep"]["batches"] == 6
    finally:
        engine.set_batch(0)


def _threshold_for_length(row, length):
    """a threshold (a double) that keeps exactly `length` entries of the row, or None when no double falls between the words
    around the boundary.  Words below 2^53 (a boundary at 256 entries is near 2^51) are exact in a double; a larger one is
    rounded down to the next double."""
    w = np.sort(row)[::-1]
    hi, lo = int(w[length - 1]), int(w[length])
    x = float(hi)
    if int(x) > hi:
        x = math.nextafter(x, 0.0)
    if not lo < int(x) <= hi:
        return None
    t = math.ldexp(x, -62)
    assert int((row >= np.uint64(R.thr_fix_of(t))).sum()) == length
    return t


def test_exact_row_lengths_and_sort_tiers(engine, tiny):
    g = tiny
    _load(engine, g, epsilon=0.5)
    cands = pick_sources(g, 6, 8300)
    want_all, _, wst_all = engine.query_fix(cands)
    try:
        for length in (256, 257, 2):
            pick = [(i, _threshold_for_length(want_all[i], length)) for i in range(len(cands))]
            i, t = next((i, t) for i, t in pick if t is not None)
            srcs, want, wst = cands[i:i + 1], want_all[i:i + 1], wst_all[i:i + 1]
            seen = []
            for cap, tile in ((None, 4096), (0, 1), (64, 64), (100, 64)):
                engine.reset_options()
                if cap is not None:
                    engine.set_option("sweep_lds_cap", cap)
                out = engine.sweep(srcs, threshold=t, want_profile=True)
                check(g, want, wst, t, 0, out)
                assert out["rows"][0]["len"] == length
                P = 1 << (length - 1).bit_length()
                assert out["sweep"]["global_rows"] == (1 if P > tile else 0)
                seen.append(_bits(out))
            assert all(b == seen[0] for b in seen)
    finally:
        engine.reset_options()


def test_sort_tiers_on_long_rows_and_max_size(engine, tiny):
    g = tiny
    _load(engine, g, epsilon=0.5)
    srcs = _mixed_sources(g, 8400)
    want, _, wst = engine.query_fix(srcs)
    try:
        seen = []
        for cap in (None, 0, 64, 1024):
            engine.reset_options()
            if cap is not None:
                engine.set_option("sweep_lds_cap", cap)
            out = engine.sweep(srcs, threshold=0.0, want_profile=True)
            check(g, want, wst, 0.0, 0, out)
            tile = {None: 4096, 0: 1}.get(cap, cap)
            P = [1 << (int(x) - 1).bit_length() if x else 0 for x in out["rows"]["len"]]
            assert out["sweep"]["global_rows"] == sum(1 for p in P if p > tile)
            if cap is not None:
                assert out["sweep"]["global_rows"] >= 1
            seen.append(_bits(out))
        assert all(b == seen[0] for b in seen)
        engine.reset_options()
        longest = int(out["rows"]["len"].max())
        assert longest > 1000
        for max_size in (1, 100, longest + 7):
            for cap in (None, 64):
                if cap is not None:
                    engine.set_option("sweep_lds_cap", cap)
                o = engine.sweep(srcs, threshold=0.0, max_size=max_size, want_profile=True)
                check(g, want, wst, 0.0, max_size, o)
                assert (np.diff(o["row_ptr"]) == np.minimum(o["rows"]["len"], max_size)).all()
                engine.reset_options()
    finally:
        engine.reset_options()


@pytest.mark.parametrize("gname", ["star", "dupes"])
def test_hubs_and_duplicate_edges(engine, request, gname):
    g = request.getfixturevalue(gname)
    _load(engine, g, epsilon=0.5)
    live = np.flatnonzero(g.deg > 0)
    srcs = np.array([0, 1, 7, 1700] if gname == "star" else live[[0, 3, 50, 3]].tolist() + [int(np.flatnonzero(g.deg == 0)[0])], dtype=np.int32)
    want, _, wst = engine.query_fix(srcs)
    for t, max_size in ((0.0, 0), (None, 0), (0.0, 40)):
        out = engine.sweep(srcs, threshold=t, max_size=max_size, want_profile=True)
        check(g, want, wst, t, max_size, out)
    if gname == "star":
        assert out["sweep"]["edges"] > 0
        full = engine.sweep(srcs, threshold=0.0, want_profile=True)
        assert 0 in full["ids"][:int(full["row_ptr"][1])] and full["sweep"]["edges"] == int(full["vol"][full["row_ptr"][1:] - 1].sum())


def test_batching_and_layouts_change_no_bit(engine, tiny_dangling):
    g = tiny_dangling
    _load(engine, g, epsilon=0.5)
    live = list(pick_sources(g, 5, 8500))
    dang = list(pick_sources(g, 2, 8501, want_dangling=True))
    srcs = np.array(live[:2] + dang[:1] + live[2:5] + dang[1:] + live[:1] + dang[:1], dtype=np.int32)
    want, _, wst = engine.query_fix(srcs)
    try:
        base = engine.sweep(srcs, want_profile=True)
        check(g, want, wst, None, 0, base)
        assert base["sweep"]["batches"] == 1
        engine.set_batch(2)
        o = engine.sweep(srcs, want_profile=True)
        assert o["sweep"]["batches"] == 3 and _bits(o) == _bits(base)
        engine.set_batch(0)
        engine.set_option("sweep_rows", 1)
        o = engine.sweep(srcs, want_profile=True)
        assert o["sweep"]["batches"] == 1 and _bits(o) == _bits(base)
        engine.set_batch(4)
        engine.set_option("sweep_rows", 3)
        o = engine.sweep(srcs, threshold=0.0, max_size=300, want_profile=True)
        check(g, want, wst, 0.0, 300, o)
        engine.set_batch(0)
        engine.reset_options()
        for layout in ({"team": 0, "tail": 0}, {"force_wide": 1}):
            for name, v in layout.items():
                engine.set_option(name, v)
            o = engine.sweep(srcs, want_profile=True)
            assert _bits(o) == _bits(base)
            for name in o["stats"].dtype.names:
                assert (o["stats"][name] == base["stats"][name]).all(), name
            engine.reset_options()
        # only dangling sources: no batch at all; no source at all
        d = np.array(dang + dang[:1], dtype=np.int32)
        o = engine.sweep(d, threshold=0.5, want_profile=True)
        assert (o["row_ptr"] == np.arange(len(d) + 1)).all() and (o["ids"] == d).all() and (o["cut"] == 0).all() and (o["vol"] == 0).all()
        assert o["sweep"]["batches"] == 0 and (o["rows"]["best"] == 0).all() and (o["rows"]["len"] == 1).all() and (o["rows"]["conductance"] == 1.0).all()
        o = engine.sweep(np.zeros(0, dtype=np.int32), want_profile=True)
        assert (o["row_ptr"] == [0]).all() and o["ids"].size == 0 and o["sweep"]["entries"] == 0 and len(o["rows"]) == 0
    finally:
        engine.set_batch(0)
        engine.reset_options()


def _raw_fetch(engine, ids, cut, vol, cap):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return engine._lib.fora_hip_sweep_fetch(engine._ctx, p(ids), p(cut), p(vol), C.c_uint64(cap))


def test_device_fetch():
    """Engine.sweep(device=True) in a child of its own (tests/sweep_device_child.py): torch tensors and the library must live
    on one HIP runtime, so the child imports torch before the library is loaded -- this process loaded the library first."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "sweep_device_child.py")], capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "sweep device ok" in r.stdout


def test_state_and_lifetime(engine, tiny):
    g = tiny
    _load(engine, g, epsilon=0.5)
    a, b = pick_sources(g, 4, 8600), pick_sources(g, 3, 8601)
    want_a, res_a, wst_a = engine.query_fix(a)
    want_b, _, wst_b = engine.query_fix(b)
    sp = engine.query_sparse(a, want_fix=True)
    oa = engine.sweep(a, want_profile=True)
    check(g, want_a, wst_a, None, 0, oa)
    # a second sweep with other sources: the rank maps were left at -1
    ob = engine.sweep(b, threshold=0.0, want_profile=True)
    check(g, want_b, wst_b, 0.0, 0, ob)
    # the dense rows afterwards are what they were
    again, res, _ = engine.query_fix(a)
    assert (again == want_a).all() and (res == res_a).all()
    # the held sparse result survived the sweeps
    e = sp[-1]["entries"]
    ids2, fix2 = np.zeros(e, np.int32), np.zeros(e, np.uint64)
    engine.sparse_fetch(ids=ids2, fix=fix2, cap=e)
    assert (ids2 == sp[1]).all() and (fix2 == sp[3]).all()
    # the held sweep survives other calls
    engine.query(a, want_ppr=False)
    sp2 = engine.query_sparse(a, threshold=1e-3, want_fix=True)   # (replaces the held sparse result, not the held sweep)
    engine.topk(a, 10)
    n_e = int(ob["row_ptr"][-1])
    ids, cut, vol = engine.sweep_fetch(n_e)
    assert (ids == ob["ids"]).all() and (cut == ob["cut"]).all() and (vol == ob["vol"]).all()
    # any subset of the outputs, a larger cap
    c3 = np.zeros(n_e + 5, np.uint64)
    assert _raw_fetch(engine, None, c3, None, n_e + 5) == 0 and (c3[:n_e] == ob["cut"]).all() and (c3[n_e:] == 0).all()
    # cap too small: refused, nothing written
    i4, c4 = np.full(n_e, -7, np.int32), np.full(n_e, 77, np.uint64)
    assert _raw_fetch(engine, i4, c4, None, n_e - 1) == -1 and (i4 == -7).all() and (c4 == 77).all()
    engine.sweep_clear()
    assert _raw_fetch(engine, i4, c4, None, n_e) == -1 and (i4 == -7).all()
    # ... and the sparse result is still there
    e2 = sp2[-1]["entries"]
    ids3, fix3 = np.zeros(e2, np.int32), np.zeros(e2, np.uint64)
    engine.sparse_fetch(ids=ids3, fix=fix3, cap=e2)
    assert 0 < e2 < e and (ids3 == sp2[1]).all() and (fix3 == sp2[3]).all()
    engine.sparse_clear()


def test_argument_errors(engine, tiny):
    g = tiny
    _load(engine, g, epsilon=0.5)
    lib, ctx = engine._lib, engine._ctx
    srcs = pick_sources(g, 2, 8700)
    held = engine.sweep(srcs, want_profile=True)
    n_e = int(held["row_ptr"][-1])
    row_ptr = np.full(3, -5, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None

    def call(src, nq, with_idx=0, thr=1.0 / g.n, rp=row_ptr):
        return lib.fora_hip_sweep_batch(ctx, p(src), C.c_int(nq), C.c_int(with_idx), C.c_double(thr), C.c_int64(0), p(rp), None, None, None)

    assert call(srcs, 2, rp=None) == -1                                     # NULL row_ptr
    # every call, failed ones too, ends the held result
    assert _raw_fetch(engine, None, None, None, n_e) == -1
    assert call(srcs, -1) == -1                                             # bad nq
    assert call(None, 2) == -1                                              # NULL sources
    assert call(np.array([0, g.n], dtype=np.int32), 2) == -1                # id out of range
    assert call(np.array([-1, 0], dtype=np.int32), 2) == -1
    assert call(srcs, 2, with_idx=1) == -1                                  # no index
    assert call(srcs, 2, thr=1.5) == -1 and call(srcs, 2, thr=float("nan")) == -1
    assert (row_ptr == -5).all()
    assert _raw_fetch(engine, None, None, None, 1 << 40) == -1              # nothing held after a failed call
    assert call(None, 0) == 0 and row_ptr[0] == 0                           # nq == 0: an empty result is held
    assert _raw_fetch(engine, None, None, None, 0) == 0
    assert call(srcs, 2) == 0 and row_ptr[0] == 0 and row_ptr[2] == n_e      # rows / stats / sweep stats may all be NULL
    ids = np.zeros(n_e, np.int32)
    assert _raw_fetch(engine, ids, None, None, n_e) == 0 and (ids == held["ids"]).all()
    engine.sweep_clear()
