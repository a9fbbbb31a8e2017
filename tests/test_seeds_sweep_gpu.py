"""Sweep cuts of seed sets on the GPU (fora_hip_seeds_sweep_batch, Engine.sweep_seeds, Engine.local_cluster_seeds): seed-set
expansion.  The expected set rows never pass through the new code: they are the Engine.query_fix rows of the individual seeds
folded by tests/seeds_ref.py; tests/sweep_ref.py -- the SWEEP CUT contract in Python ints -- sweeps them.  Everything is
asserted equal: row_ptr, the rows (len, best, cut, vol, den, conductance bit for bit) and the fetched order / cut / vol."""
import ctypes as C

import numpy as np
import pytest

import seeds_outputs_ref as so
import seeds_ref as sr
import sweep_ref as R
from fora_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def odd(oracle):
    """n odd: every other row of the accumulator block starts at an odd word (no 16-byte alignment)."""
    src, dst = synth.rmat_graph(1999, 16000, 20260118)
    return oracle.Graph.from_edges(1999, 16000, src, dst)


_MEMO = {}


def _ref(g, key, row, thr, max_size):
    """the twin of one expected row, computed once per (graph, row, threshold, max_size)"""
    key = (id(g), key, thr, max_size)
    full = _MEMO.get(key[:3] + (0,))
    if max_size > 0 and full is not None and full["len"] <= max_size:
        return full   # (nothing is cut off: the uncut profile, already computed)
    if key not in _MEMO:
        _MEMO[key] = R.sweep_row(np.array(row, dtype=np.uint64), g.row_ptr, g.col, thr, max_size)
    return _MEMO[key]


def check(g, tag, sets, expect, t, max_size, out, dedup=1):
    """one call's dict (with its profile) against the expected set rows; tag names the rows for the memo"""
    thr = so.thr_fix_of(1.0 / g.n if t is None else t)
    ns = len(expect)
    row_ptr, rows, ids, cut, vol = out["row_ptr"], out["rows"], out["ids"], out["cut"], out["vol"]
    assert row_ptr.dtype == np.int64 and row_ptr.shape == (ns + 1,) and row_ptr[0] == 0 and len(rows) == ns
    assert ids.dtype == np.int32 and cut.dtype == np.uint64 and vol.dtype == np.uint64
    assert ids.shape == cut.shape == vol.shape == (int(row_ptr[-1]),)
    entries = longest = 0
    for i in range(ns):
        r = _ref(g, (tag, i), expect[i], thr, max_size)
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
    for name, want in so.counts(g, sets, dedup).items():
        assert out["stats"][name] == want, name
    sw = out["sweep"]
    assert sw["entries"] == entries and sw["max_row"] == longest and sw["thr_fix"] == thr
    assert sw["compact_ms"] >= 0.0 and sw["sort_ms"] >= 0.0 and sw["cut_ms"] >= 0.0


def both(engine, g, c, t=None, max_size=0, dedup=1, with_idx=False):
    for k, w in (("u", None), ("w", c.weights)):
        out = engine.sweep_seeds(c.sets, weights=w, with_idx=with_idx, threshold=t, max_size=max_size, want_profile=True)
        check(g, (k, with_idx), c.sets, c.expect[k], t, max_size, out, dedup)
    return out


def _bits(out):
    return (out["row_ptr"].tobytes(), out["rows"].tobytes(), out["ids"].tobytes(), out["cut"].tobytes(), out["vol"].tobytes())


@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling", "odd"])
def test_sweep_equals_the_twin_of_the_set_rows(engine, request, gname):
    g = request.getfixturevalue(gname)
    so.load(engine, g)
    c = so.reference(engine, g)
    for t in (None, 0.0, 1e-3):
        out = both(engine, g, c, t)
    for max_size in (1, 50):
        for t in (None, 0.0):
            o = both(engine, g, c, t, max_size)
            assert (np.diff(o["row_ptr"]) == np.minimum(o["rows"]["len"], max_size)).all()
    assert (out["rows"]["len"] > 0).all()
    if gname == "tiny_dangling":   # the set of dangling seeds only: its support is those seeds, no prefix has a volume
        i = 3
        assert all(g.deg[s] == 0 for s in c.sets[i])
        full = engine.sweep_seeds(c.sets, threshold=0.0, want_profile=True)
        lo, hi = int(full["row_ptr"][i]), int(full["row_ptr"][i + 1])
        assert sorted(full["ids"][lo:hi].tolist()) == sorted(set(c.sets[i])) and (full["vol"][lo:hi] == 0).all() and (full["cut"][lo:hi] == 0).all()
        r = full["rows"][i]
        assert (int(r["len"]), int(r["best"]), int(r["cut"]), int(r["vol"]), int(r["den"])) == (hi - lo, 0, 0, 0, 0) and r["conductance"] == 1.0
    # the best clusters, by the public call
    o = engine.sweep_seeds(c.sets, weights=c.weights, want_profile=True)
    members = engine.local_cluster_seeds(c.sets, weights=c.weights)
    assert len(members) == len(c.sets)
    for i, m in enumerate(members):
        lo = int(o["row_ptr"][i])
        assert m.dtype == np.int32 and m.tolist() == o["ids"][lo:lo + int(o["rows"][i]["best"])].tolist()
    assert any(m.size > 0 for m in members)


def test_a_singleton_equals_sweep(engine, tiny_dangling):
    g = tiny_dangling
    so.load(engine, g)
    live, dang = so.pick(g, 3, 621), so.pick(g, 2, 622, want_dangling=True)
    srcs = live[:2] + dang[:1] + live[2:] + dang[1:]
    assert len(dang) == 2
    for t, max_size in ((None, 0), (0.0, 0), (0.0, 50)):
        want = engine.sweep(np.array(srcs, dtype=np.int32), threshold=t, max_size=max_size, want_profile=True)
        out = engine.sweep_seeds([[s] for s in srcs], threshold=t, max_size=max_size, want_profile=True)
        assert _bits(out) == _bits(want)
        for name in ("entries", "max_row", "thr_fix", "edges", "global_rows"):
            assert out["sweep"][name] == want["sweep"][name], name
        for i, s in enumerate(srcs):
            if g.deg[s] == 0:   # a dangling seed: len 1, best 0, the profile entry (s, 0, 0)
                lo = int(out["row_ptr"][i])
                assert int(out["row_ptr"][i + 1]) == lo + 1 and (int(out["ids"][lo]), int(out["cut"][lo]), int(out["vol"][lo])) == (s, 0, 0)
                assert (int(out["rows"][i]["len"]), int(out["rows"][i]["best"])) == (1, 0) and out["rows"][i]["conductance"] == 1.0


@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling", "odd"])
@pytest.mark.parametrize("cap", [None, 64, 0])
def test_sort_tiers_change_no_bit(engine, request, gname, cap):
    g = request.getfixturevalue(gname)
    so.load(engine, g)
    c = so.reference(engine, g)
    try:
        if cap is not None:
            engine.set_option("sweep_lds_cap", cap)
        out = both(engine, g, c, 0.0)
        tile = {None: 4096, 0: 1}.get(cap, cap)
        P = [1 << (int(x) - 1).bit_length() if x else 0 for x in out["rows"]["len"]]
        assert out["sweep"]["global_rows"] == sum(1 for p in P if p > tile)
        if cap == 64:
            assert out["sweep"]["global_rows"] >= 1   # the supports reach the global tier
        both(engine, g, c, None, 50)
    finally:
        engine.reset_options()


@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling", "odd"])
@pytest.mark.parametrize("sweep_rows", [1, 3])
@pytest.mark.parametrize("seeds_rows", [1, 3, 256])
def test_chunks_of_rows_change_no_bit(engine, request, gname, sweep_rows, seeds_rows):
    """seeds_rows bounds the rows compacted and sorted at a time, sweep_rows the rank maps inside such a chunk.  seeds_rows 1
    and 3 on the graph of 1999 nodes are the alignment rule's case."""
    g = request.getfixturevalue(gname)
    so.load(engine, g)
    c = so.reference(engine, g)
    try:
        engine.set_option("sweep_rows", sweep_rows)
        engine.set_option("seeds_rows", seeds_rows)
        out = both(engine, g, c, None)
        rows = seeds_rows + (seeds_rows & g.n & 1)   # an odd n: rounded up to even
        assert out["sweep"]["batches"] == -(-len(c.sets) // rows)
        both(engine, g, c, 0.0, 50)
    finally:
        engine.reset_options()


@pytest.mark.parametrize("gname", ["tiny_dangling", "odd"])
@pytest.mark.parametrize("batch,dedup,wide", [(4, 1, False), (4, 0, True), (1, 1, False)])
def test_batching_dedup_and_layout_change_no_bit(engine, request, gname, batch, dedup, wide):
    g = request.getfixturevalue(gname)
    so.load(engine, g)
    c = so.reference(engine, g)
    try:
        if wide:
            engine.set_option("force_wide", 1)
        engine.set_option("seeds_dedup", dedup)
        engine.set_batch(batch)
        out = both(engine, g, c, None, dedup=dedup)
        if batch == 4:
            assert out["stats"]["batches"] == -(-out["stats"]["queries"] // 4) >= 3
    finally:
        engine.reset_options()
        engine.set_batch(0)


@pytest.mark.parametrize("batch", [0, 4])
def test_with_idx_rows_come_from_the_indexed_queries(engine, tiny_dangling, batch):
    g = tiny_dangling
    so.load(engine, g)
    try:
        engine.build_index()
        c = so.reference(engine, g, with_idx=True)
        engine.set_batch(batch)
        both(engine, g, c, None, with_idx=True)
    finally:
        engine.set_batch(0)
        engine.clear_index()


def test_long_rows_on_the_global_tier(engine, small):
    """Two 3-seed sets on 32 000 nodes at the default tile: supports of more than 16 384 entries, padded to P = 32768."""
    g = small
    so.load(engine, g)
    seeds = so.pick(g, 6, 631)
    sets = [seeds[:3], seeds[3:]]
    fix, _, _ = engine.query_fix(np.array(seeds, dtype=np.int32), want_residue=False)
    expect = [sr.combine([fix[j].tolist() for j in range(3 * i, 3 * i + 3)], sr.uniform_wfix(3)) for i in range(2)]
    out = engine.sweep_seeds(sets, threshold=0.0, want_profile=True)
    check(g, "long", sets, expect, 0.0, 0, out)
    assert (out["rows"]["len"] > 16384).all() and (out["rows"]["len"] <= 32768).all()
    assert out["sweep"]["global_rows"] == 2


def _raw_fetch(engine, ids, cut, vol, cap):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return engine._lib.fora_hip_sweep_fetch(engine._ctx, p(ids), p(cut), p(vol), C.c_uint64(cap))


def test_state_and_lifetime(engine, tiny_dangling):
    g = tiny_dangling
    so.load(engine, g)
    c = so.reference(engine, g)
    srcs = np.array(c.sets[-1][:4], dtype=np.int32)
    want, _, _ = engine.query_fix(srcs, want_residue=False)
    sp = engine.query_sparse(srcs, want_fix=True)
    first = engine.sweep(srcs, want_profile=True)
    out = engine.sweep_seeds(c.sets, want_profile=True)   # replaces the held profile
    check(g, ("u", False), c.sets, c.expect["u"], None, 0, out)
    n_e = int(out["row_ptr"][-1])
    assert n_e != int(first["row_ptr"][-1])
    # the rank block was left all -1: a following sweep equals its own twin
    after = engine.sweep(srcs, threshold=0.0, want_profile=True)
    thr = so.thr_fix_of(0.0)
    for i in range(len(srcs)):
        r = R.sweep_row(want[i], g.row_ptr, g.col, thr, 0)
        lo, hi = int(after["row_ptr"][i]), int(after["row_ptr"][i + 1])
        assert after["ids"][lo:hi].tolist() == r["order"] and after["cut"][lo:hi].tolist() == r["cut"] and after["vol"][lo:hi].tolist() == r["vol"]
        assert (int(after["rows"][i]["len"]), int(after["rows"][i]["best"])) == (r["len"], r["best"])
    out = engine.sweep_seeds(c.sets, want_profile=True)
    # the sparse result held before the calls is untouched by them
    e = sp[-1]["entries"]
    ids2, fix2 = np.zeros(e, np.int32), np.zeros(e, np.uint64)
    engine.sparse_fetch(ids=ids2, fix=fix2, cap=e)
    assert (ids2 == sp[1]).all() and (fix2 == sp[3]).all()
    # the held profile survives other calls, the seed sets' other two among them
    engine.query(srcs, want_ppr=False)
    engine.query_seeds(c.sets, want_fix=False)
    engine.query_seeds_sparse(c.sets[:3])
    ids, cut, vol = engine.sweep_fetch(n_e)
    assert (ids == out["ids"]).all() and (cut == out["cut"]).all() and (vol == out["vol"]).all()
    c3 = np.zeros(n_e + 5, np.uint64)
    assert _raw_fetch(engine, None, c3, None, n_e + 5) == 0 and (c3[:n_e] == out["cut"]).all() and (c3[n_e:] == 0).all()
    # cap too small: refused, nothing written
    i4, c4 = np.full(n_e, -7, np.int32), np.full(n_e, 77, np.uint64)
    assert _raw_fetch(engine, i4, c4, None, n_e - 1) == -1 and (i4 == -7).all() and (c4 == 77).all()
    engine.sweep_clear()
    assert _raw_fetch(engine, i4, c4, None, n_e) == -1 and (i4 == -7).all()
    engine.sparse_clear()


def _raw(engine, set_ptr, seeds, weights, ns, with_idx=0, thr=0.0, row_ptr=None):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return engine._lib.fora_hip_seeds_sweep_batch(engine._ctx, p(set_ptr), p(seeds), p(weights), C.c_int(ns), C.c_int(with_idx),
                                                  C.c_double(thr), C.c_int64(0), p(row_ptr), None, None, None)


def test_argument_errors_and_the_empty_call(engine, tiny):
    g = tiny
    so.load(engine, g)
    a, b = so.pick(g, 2, 604)
    good = engine.sweep_seeds([[a, b]], want_profile=True)
    n_e = int(good["row_ptr"][-1])
    i64 = lambda *x: np.array(x, dtype=np.int64)
    i32 = lambda *x: np.array(x, dtype=np.int32)
    f64 = lambda *x: np.array(x, dtype=np.float64)
    rp = np.full(4, -5, dtype=np.int64)
    cases = {
        "null row_ptr": (i64(0, 1), i32(a), None, 1, 0, 0.0, None),
        "threshold > 1": (i64(0, 1), i32(a), None, 1, 0, 1.5, rp),
        "threshold nan": (i64(0, 1), i32(a), None, 1, 0, float("nan"), rp),
        "ns < 0": (i64(0, 1), i32(a), None, -1, 0, 0.0, rp),
        "null set_ptr": (None, i32(a), None, 1, 0, 0.0, rp),
        "null seeds": (i64(0, 1), None, None, 1, 0, 0.0, rp),
        "set_ptr[0] != 0": (i64(1, 2), i32(a, b), None, 1, 0, 0.0, rp),
        "decreasing set_ptr": (i64(0, 2, 1), i32(a, b), None, 2, 0, 0.0, rp),
        "empty set": (i64(0, 0, 1), i32(a), None, 2, 0, 0.0, rp),
        "seed == n": (i64(0, 2), i32(a, g.n), None, 1, 0, 0.0, rp),
        "seed < 0": (i64(0, 2), i32(-1, a), None, 1, 0, 0.0, rp),
        "negative weight": (i64(0, 2), i32(a, b), f64(1.0, -0.5), 1, 0, 0.0, rp),
        "zero sum": (i64(0, 1, 3), i32(a, a, b), f64(1.0, 0.0, 0.0), 2, 0, 0.0, rp),
        "with_idx without an index": (i64(0, 1), i32(a), None, 1, 1, 0.0, rp),
    }
    for name, (set_ptr, seeds, weights, ns, with_idx, thr, row_ptr) in cases.items():
        assert _raw(engine, set_ptr, seeds, weights, ns, with_idx, thr, row_ptr) == -1, name  # FORA_E_ARG
        assert (rp == -5).all(), name
        assert _raw_fetch(engine, None, None, None, 1 << 40) == -1, name   # every call, a failed one too, ends the held result
    later = engine.sweep_seeds([[a, b]], want_profile=True)   # a later correct call is what it was
    assert _bits(later) == _bits(good)
    # ns == 0: an empty result is held, the stats are zero
    out = engine.sweep_seeds([], want_profile=True)
    assert out["row_ptr"].tolist() == [0] and out["ids"].size == 0 and len(out["rows"]) == 0
    assert all(v == 0 for v in out["stats"].values()) and all(v == 0 for v in out["sweep"].values())
    assert _raw_fetch(engine, None, None, None, 0) == 0
    assert _raw(engine, None, None, None, 0, row_ptr=rp) == 0 and rp[0] == 0   # nothing to read: null arrays are fine
    engine.sweep_clear()
    assert _raw_fetch(engine, None, None, None, n_e) == -1
