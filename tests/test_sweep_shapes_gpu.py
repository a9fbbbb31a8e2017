"""The sweep kernels (fora_sweep.h) on the inputs real PPR rows of small graphs never reach: rows longer than a sort tile and
than one trip of a grid-stride loop, equal keys across every tile boundary, equal conductances, crowded degree classes, and
k_sweep_scan alone on 128-bit products.  DESIGN.md 5.10 lists which gap each test closes.

Every assertion is equality with tests/sweep_ref.py through check() of tests/test_sweep_gpu.py: the public call against the
dense rows of the same context, rows put in through the TEST ENTRY POINTS of include/fora_hip.h (libfora_hip_test.so) against
the rows themselves.  Each test asserts on the reference's output that its input has the property it is there for."""
import numpy as np
import pytest

import sweep_ref as R
from conftest import pick_sources
from test_sweep_gpu import G, _bits, _load, _ref, check

pytestmark = pytest.mark.gpu


def _P(length):
    return 1 << (int(length) - 1).bit_length() if length else 0


def _sources(g, seed):
    """six sources: four live ones, a dangling one where the graph has one (a fifth live one otherwise), one live one twice"""
    live = list(pick_sources(g, 5, seed))
    dang = list(pick_sources(g, 1, seed + 1, want_dangling=True))
    return np.array(live[:2] + (dang or live[4:]) + live[2:4] + live[1:2], dtype=np.int32)


@pytest.mark.parametrize("gname", ["small", "small_dangling"])
def test_public_call_at_the_default_tier(engine, request, gname):
    g = request.getfixturevalue(gname)
    srcs = _sources(g, 8800)
    live = g.deg[srcs] > 0
    assert len(srcs) == 6 and len(set(srcs.tolist())) == 5 and int((~live).sum()) == (1 if gname == "small_dangling" else 0)
    _load(engine, g, epsilon=0.5)
    want, _, wst = engine.query_fix(srcs)
    try:
        # thresholds, at the default tile of 4096 entries
        for t in (0.0, None, 1e-3):
            out = engine.sweep(srcs, threshold=t, want_profile=True)
            check(g, want, wst, t, 0, out)
        # sort tiers on rows of more than one tile
        seen = []
        for cap in (None, 64, 0):
            engine.reset_options()
            if cap is not None:
                engine.set_option("sweep_lds_cap", cap)
            out = engine.sweep(srcs, threshold=0.0, want_profile=True)
            check(g, want, wst, 0.0, 0, out)
            tile = {None: 4096, 0: 1}.get(cap, cap)
            P = [_P(x) for x in out["rows"]["len"]]
            assert out["sweep"]["global_rows"] == sum(1 for i, p in enumerate(P) if live[i] and p > tile)
            if cap is None:
                assert max(P) > 4096 and out["sweep"]["global_rows"] >= 1
            seen.append(_bits(out))
        assert all(b == seen[0] for b in seen)
        engine.reset_options()
        # several batches, the rank maps of one and of three rows at a time: the held arrays grow with profiles in them
        engine.set_batch(2)
        for rows_at_a_time in (1, 3):
            engine.set_option("sweep_rows", rows_at_a_time)
            o = engine.sweep(srcs, threshold=0.0, want_profile=True)
            assert o["sweep"]["batches"] == (int(live.sum()) + 1) // 2 and _bits(o) == seen[0]
        engine.set_batch(0)
        engine.reset_options()
        # profiles cut off at, below and above a tile, and not at all
        longest = int(out["rows"]["len"].max())
        for max_size in (1, 4096, 4097, longest + 7):
            o = engine.sweep(srcs, threshold=0.0, max_size=max_size, want_profile=True)
            check(g, want, wst, 0.0, max_size, o)
            assert (np.diff(o["row_ptr"]) == np.minimum(o["rows"]["len"], max_size)).all()
        if gname == "small":   # once with the index
            engine.build_index()
            want_i, _, wst_i = engine.query_fix(srcs[:3], with_idx=True)
            out = engine.sweep(srcs[:3], with_idx=True, threshold=0.0, want_profile=True)
            check(g, want_i, wst_i, 0.0, 0, out)
            assert out["sweep"]["global_rows"] == 3
    finally:
        engine.set_batch(0)
        engine.reset_options()
        engine.clear_index()


def _inject(e, g, rows, t=0.0, max_size=0):
    """rows through fora_hip_test_sweep_rows, held to the twin of the rows themselves"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, g.n)
    out = e.test_sweep_rows(rows, threshold=t, max_size=max_size)
    check(g, rows, None, t, max_size, out)
    return out


def _tiers(e, g, rows, t=0.0, max_size=0):
    """_inject under the default tile, tiles of 64 and no tile at all: the same bits; returns the default's result"""
    seen = []
    try:
        for cap in (None, 64, 0):
            e.reset_options()
            if cap is not None:
                e.set_option("sweep_lds_cap", cap)
            out = _inject(e, g, rows, t, max_size)
            tile = {None: 4096, 0: 1}.get(cap, cap)
            assert out["sweep"]["global_rows"] == sum(1 for x in out["rows"]["len"] if _P(x) > tile)
            seen.append((out, _bits(out)))
    finally:
        e.reset_options()
    assert all(b == seen[0][1] for _, b in seen)
    return seen[0][0]


def test_equal_keys_across_every_tile_boundary(engine_test, small_dangling):
    g = small_dangling
    _load(engine_test, g, epsilon=0.5)
    nnz = int(g.row_ptr[-1])
    long_rows = [R.tie_heavy_row(g.n, g.row_ptr, s) for s in R.TIE_SEEDS]
    single = np.zeros(g.n, dtype=np.uint64)
    single[int(np.flatnonzero(g.deg > 0)[5])] = 7 << 50
    rows = long_rows + [R.row_of_length(long_rows[0], k) for k in (4096, 4097, 8192)] + [np.zeros(g.n, dtype=np.uint64), single]
    # what the rows are there for, on the reference
    conductance_ties = 0
    for i, row in enumerate(rows[:6]):
        r = _ref(g, row, 1, 0)
        keys = R.keys_in_order(row, g.row_ptr, r["order"])
        tied = [R.tied_boundaries(keys, s) for s in (64, 1024, 4096)]
        assert len(set(keys)) == 5 and tied[1][0] == tied[1][1] and tied[2][0] == tied[2][1] and tied[0][0] >= tied[0][1] - 1
        if i < 3:
            assert r["len"] > 6 * 4096 and tied[1] == (24, 24) and tied[2] == (6, 6)
            conductance_ties += len(R.minimisers(r["cut"], r["vol"], nnz)) > 1
        if i == 0:
            assert tied[0][0] == tied[0][1] >= 398
    assert conductance_ties >= 1
    assert [_ref(g, row, 1, 0)["len"] for row in rows[3:]] == [4096, 4097, 8192, 0, 1]
    try:
        out = _tiers(engine_test, g, rows)
        assert out["rows"]["len"].tolist() == [_ref(g, row, 1, 0)["len"] for row in rows] and out["sweep"]["batches"] == 1
        assert out["rows"]["best"][6] == 0 and out["rows"]["best"][7] == 1 and out["sweep"]["global_rows"] == 5
        # the empty row, the one-entry row and a long one in every batch of three; the rank map of one row at a time
        mixed = [rows[6], rows[7], rows[1], rows[2], rows[6], rows[7]]
        engine_test.set_batch(3)
        engine_test.set_option("sweep_rows", 1)
        o = _inject(engine_test, g, mixed)
        assert o["sweep"]["batches"] == 2 and o["rows"]["len"].tolist() == [0, 1, out["rows"]["len"][1], out["rows"]["len"][2], 0, 1]
        engine_test.set_batch(0)
        engine_test.reset_options()
        # a threshold and a cut-off on the tied rows: the support ends inside a run of equal keys
        _inject(engine_test, g, rows[:2], t=float(3 << 40) / float(1 << 62), max_size=5000)
    finally:
        engine_test.set_batch(0)
        engine_test.reset_options()


def test_words_at_the_edges_of_the_key(engine_test, small_dangling):
    g = small_dangling
    _load(engine_test, g, epsilon=0.5)
    row, zero = R.edge_words_row(g.n, g.row_ptr, 8810)
    r = _ref(g, row, 1, 0)
    keys = R.keys_in_order(row, g.row_ptr, r["order"])
    nz = zero.size
    assert nz == 1200 and r["len"] == 4801 and _P(r["len"]) == 8192            # pads behind the key-0 entries, two tiles
    assert keys[0] == R.FIX_ONE and g.deg[r["order"][0]] == 1
    assert keys[-nz:] == [0] * nz and keys[-nz - 1] == 1 and r["order"][-nz:] == zero.tolist()   # key 0: last, by id
    assert len({k >> 33 for k in keys if k & 0xFFFFFFFF == 12345}) == 7 and len({k for k in keys if k >> 33 == 9}) > 1000
    out = _tiers(engine_test, g, [row])
    assert out["rows"]["len"][0] == r["len"] and out["ids"][-nz:].tolist() == zero.tolist() and (out["ids"] < g.n).all()
    _inject(engine_test, g, [row], max_size=r["len"] - nz + 3)   # cut off inside the key-0 run


def test_degree_classes_crowd_one_block(engine_test, small_dangling):
    g = small_dangling
    _load(engine_test, g, epsilon=0.5)
    row = R.hubs_first_row(g.row_ptr)
    d = g.deg[_ref(g, row, 1, 4000)["order"][:256]]
    assert (int((d >= 256).sum()), int(((d >= 64) & (d < 256)).sum())) == R.HUB_CLASSES == (121, 135)
    for max_size in (0, 4000):
        out = _inject(engine_test, g, [row], max_size=max_size)
        assert out["rows"]["len"][0] == g.n and int(out["row_ptr"][1]) == (max_size or g.n)
    assert out["sweep"]["edges"] == int(g.deg[out["ids"]].sum())


@pytest.fixture(scope="module")
def chord_ring():
    n, row_ptr, col = R.chord_ring_graph()
    g = G(n, row_ptr, col)
    assert g.n == 40000 and g.deg[0] >= 256 and (g.deg >= 2).all()
    return g


def test_grid_stride_loops_take_a_second_trip(engine_test, chord_ring):
    g = chord_ring
    _load(engine_test, g, epsilon=0.5)
    row = R.hubs_first_row(g.row_ptr)
    r = _ref(g, row, 1, 0)
    assert r["len"] == g.n > 32768 and _P(r["len"]) == 65536 and r["order"][0] == 0
    out = _inject(engine_test, g, [row])
    assert out["rows"]["len"][0] == g.n and out["sweep"]["global_rows"] == 1
    # two rows in the batch, the second short: the grids are sized by the longer one
    _inject(engine_test, g, [row, R.row_of_length(row, 300)], max_size=33000)


@pytest.mark.parametrize("m", [9, 513, 2049, 8193, "pairs"])
def test_equal_conductances_go_to_the_smaller_prefix(engine_test, m):
    n, row_ptr, col, row = R.pair_graph(3000) if m == "pairs" else R.ring_graph(m)
    g = G(n, row_ptr, col)
    _load(engine_test, g, epsilon=0.5)
    r = _ref(g, row, 1, 0)
    ms = R.minimisers(r["cut"], r["vol"], g.m)
    want = list(range(1, 5999, 2)) if m == "pairs" else {9: [3, 4], 513: [255, 256], 2049: [1023, 1024], 8193: [4095, 4096]}[m]
    assert ms == want and len(ms) >= 2 and r["best"] == ms[0] + 1 and r["order"] == list(range(n))
    out = _tiers(engine_test, g, [row]) if m == 8193 else _inject(engine_test, g, [row])
    assert int(out["rows"]["best"][0]) == ms[0] + 1
    if m != "pairs":   # cut off between the two, and right behind them
        for max_size in (ms[0] + 1, ms[1] + 1):
            o = _inject(engine_test, g, [row], max_size=max_size)
            assert int(o["rows"]["best"][0]) == ms[0] + 1


def test_injected_rows_give_the_bits_of_the_public_call(engine, engine_test, tiny):
    g = tiny
    srcs = pick_sources(g, 3, 8820)
    _load(engine, g, epsilon=0.5)
    want, _, wst = engine.query_fix(srcs)
    _load(engine_test, g, epsilon=0.5)
    for t, max_size in ((None, 0), (0.0, 100)):
        pub = engine.sweep(srcs, threshold=t, max_size=max_size, want_profile=True)
        check(g, want, wst, t, max_size, pub)
        inj = engine_test.test_sweep_rows(want, threshold=t, max_size=max_size)
        assert _bits(inj) == _bits(pub)
        for k in ("entries", "max_row", "thr_fix", "edges", "batches", "global_rows"):
            assert inj["sweep"][k] == pub["sweep"][k], k


def test_injected_calls_leave_no_trace(engine_test, tiny):
    g = tiny
    _load(engine_test, g, epsilon=0.5)
    srcs = pick_sources(g, 4, 8830)
    before = engine_test.query_fix(srcs)
    a = [R.tie_heavy_row(g.n, g.row_ptr, 8831), R.hubs_first_row(g.row_ptr)]
    b = [R.tie_heavy_row(g.n, g.row_ptr, 8832), np.zeros(g.n, dtype=np.uint64), R.edge_words_row(g.n, g.row_ptr, 8833, count=100)[0]]
    _inject(engine_test, g, a)
    held = _inject(engine_test, g, b, max_size=700)   # other rows, other lengths: the rank maps were left at -1
    ids, cut, vol = engine_test.sweep_fetch(int(held["row_ptr"][-1]))
    after = engine_test.query_fix(srcs)
    assert (after[0] == before[0]).all() and (after[1] == before[1]).all()
    for name in after[2].dtype.names:
        assert (after[2][name] == before[2][name]).all(), name
    # the profile an injected call left is held like any other
    again = engine_test.sweep_fetch(int(held["row_ptr"][-1]))
    assert (again[0] == ids).all() and (again[1] == cut).all() and (again[2] == vol).all() and (ids == held["ids"]).all()
    pub = engine_test.sweep(srcs, want_profile=True)
    check(g, before[0], before[2], None, 0, pub)


def _scan(e, diff, vol, nnz):
    """k_sweep_scan through fora_hip_test_sweep_scan against Python ints: both scans, best, cut, vol, den, edges"""
    ref = R.scan_ref(diff, vol, nnz)
    cut, vs, o = e.test_sweep_scan(diff, vol, nnz)
    assert cut.dtype == np.uint64 and vs.dtype == np.uint64
    assert cut.tolist() == ref["cut"] and vs.tolist() == ref["vol"]
    assert (o["len"], o["best"], o["cut"], o["vol"], o["den"], o["edges"]) == \
           (len(diff), ref["best"], ref["cut_best"], ref["vol_best"], ref["den"], ref["edges"])
    return ref


@pytest.mark.parametrize("L", R.SCAN_LENGTHS)
def test_scan_and_argmin_on_128_bit_products(engine_test, tiny, L):
    _load(engine_test, tiny, epsilon=0.5)   # (any graph: the entry point takes nnz as an argument)
    rng = np.random.Generator(np.random.PCG64(8840 + L))
    seen = 0
    for kind in R.SCAN_KINDS:
        for p, q in R.SCAN_PLACES.values():
            if q >= L:
                continue
            diff, vol, nnz, winner = R.scan_planted(rng, L, kind, p, q)
            pre = R.scan_ref(diff, vol, nnz)
            assert R.minimisers(pre["cut"], pre["vol"], nnz) == ([p, q] if kind == "tie" else [winner]) and pre["best"] == winner + 1
            assert pre["cut"][p] * pre["vol"][q] >> 64 and max(pre["cut"]) <= 1 << 45 and int(diff.min()) < -(1 << 40) and int(vol.max()) <= 1 << 40
            ref = _scan(engine_test, diff, vol, nnz)
            assert ref["best"] == winner + 1
            seen += 1
    assert seen == {1: 0, 4: 5, 5: 5, 1024: 15, 1025: 20, 5000: 25}[L]
    # denominators from both sides of nnz / 2, none at the last prefix (L == 1: none at all); then some at every prefix
    diff, vol, nnz = R.scan_plain(rng, L)
    ref = _scan(engine_test, diff, vol, nnz)
    assert ref["edges"] == nnz and (ref["best"] == 0) == (L == 1)
    assert _scan(engine_test, *R.scan_plain(rng, L, 12345))["best"] > 0
    # no prefix with a denominator
    ref = _scan(engine_test, np.ones(L, np.int64), np.zeros(L, np.uint64), 77)
    assert (ref["best"], ref["den"], ref["edges"]) == (0, 0, 0)
    # the held profile of an earlier call is not the scan's buffer
    row = R.hubs_first_row(tiny.row_ptr)
    held = _inject(engine_test, tiny, [row])
    _scan(engine_test, *R.scan_plain(rng, L))
    ids, cut, vs = engine_test.sweep_fetch(int(held["row_ptr"][-1]))
    assert (ids == held["ids"]).all() and (cut == held["cut"]).all() and (vs == held["vol"]).all()
