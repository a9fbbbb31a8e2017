"""The SWEEP CUT contract (include/fora_hip.h) on the CPU: tests/sweep_ref.py, the Python twin the GPU tests compare with,
against a brute force over set membership; the cases without a best prefix; the tie rule; the recovery of a planted block on
rows of the oracle's twin; the C ABI's new symbols and structs; and the generators of tests/test_sweep_shapes_gpu.py's inputs
(tie-heavy and hubs-first rows, rings, pairs, inputs of k_sweep_scan), each against the brute force and for the property the
GPU test relies on.  The two test-only entry points must be in libfora_hip_test.so and nowhere else.  Last, the host-side plan
of a sweep batch (fora_amd/csrc/fora_sweep_plan.h) against tests/sweep_plan_check.cpp's brute force, under the sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import sweep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX_ONE = 1 << 62


def _random_graph(rng, n, dup=True):
    """directed, with duplicate edges and dangling nodes, no self loops"""
    deg = rng.integers(0, 7, size=n)
    deg[rng.choice(n, size=max(1, n // 6), replace=False)] = 0
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=row_ptr[1:])
    col = np.zeros(int(row_ptr[-1]), dtype=np.int32)
    for u in range(n):
        t = rng.integers(0, n - 1, size=deg[u])
        t = t + (t >= u)  # no self loop
        if dup and deg[u] >= 2:
            t[1] = t[0]   # a stored duplicate
        col[row_ptr[u]:row_ptr[u + 1]] = t
    return row_ptr, col


def _same(a, b):
    for k in ("len", "order", "cut", "vol", "best", "cut_best", "vol_best", "den"):
        assert a[k] == b[k], k
    assert R.f64_bits(a["conductance"]) == R.f64_bits(b["conductance"])


@pytest.mark.parametrize("seed", range(6))
def test_twin_equals_brute_force(seed):
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    n = int(rng.integers(30, 201))
    row_ptr, col = _random_graph(rng, n)
    deg = np.diff(row_ptr)
    assert (deg == 0).any() and any(col[row_ptr[u]] == col[row_ptr[u] + 1] for u in range(n) if deg[u] >= 2)
    for _ in range(3):
        row = R.random_row(rng, n, row_ptr)
        full = R.sweep_row(row, row_ptr, col, 1)
        keys = [int(row[v]) // max(int(deg[v]), 1) for v in full["order"]]
        assert keys == sorted(keys, reverse=True) and len(set(keys)) < len(keys)          # equal keys ...
        assert all(a < b for a, b, ka, kb in zip(full["order"], full["order"][1:], keys, keys[1:]) if ka == kb)  # ... tie by id
        assert (row[full["order"]] > 0).all() and full["len"] == int((row > 0).sum())
        for thr in (1, 3 << 40):
            for max_size in (0, 1, full["len"] // 2, full["len"] + 5):
                a = R.sweep_row(row, row_ptr, col, thr, max_size)
                _same(a, R.sweep_brute(row, row_ptr, col, thr, max_size))
                assert len(a["order"]) == (a["len"] if max_size <= 0 else min(a["len"], max_size))
                assert a["order"] == R.sweep_row(row, row_ptr, col, thr)["order"][:len(a["order"])]


def test_rows_without_a_best_prefix():
    # 0 -> 1, 1 -> 0, 0 -> 2 ; 2 and 3 dangling
    row_ptr = np.array([0, 2, 3, 3, 3], dtype=np.int64)
    col = np.array([1, 2, 0], dtype=np.int32)
    none = dict(best=0, cut_best=0, vol_best=0, den=0, conductance=1.0)

    def check(r, length):
        assert r["len"] == length
        for k, v in none.items():
            assert r[k] == v, k

    check(R.sweep_row(np.zeros(4, dtype=np.uint64), row_ptr, col, 1), 0)                        # an empty row
    check(R.dangling_row(2), 1)                                                                # a dangling source
    r = R.sweep_row(np.array([0, 0, 5, 9], dtype=np.uint64), row_ptr, col, 1)                  # dangling nodes only
    check(r, 2)
    assert r["order"] == [3, 2] and r["cut"] == [0, 0] and r["vol"] == [0, 0]
    # vol == nnz: one node holds every edge
    row_ptr1 = np.array([0, 2, 2, 2], dtype=np.int64)
    col1 = np.array([1, 2], dtype=np.int32)
    r = R.sweep_row(np.array([8, 0, 0], dtype=np.uint64), row_ptr1, col1, 1)
    check(r, 1)
    assert r["cut"] == [2] and r["vol"] == [2]
    # ... while a row over the first graph that reaches vol == nnz only at its end has a best prefix before it
    r = R.sweep_row(np.array([8, 8, 1, 0], dtype=np.uint64), row_ptr, col, 1)
    assert r["order"] == [1, 0, 2] and r["vol"] == [1, 3, 3] and r["cut"] == [1, 1, 0] and (r["best"], r["cut_best"], r["den"]) == (1, 1, 1)


def test_conductance_ties_go_to_the_smaller_prefix():
    # two disjoint 2-cycles {0, 1}, {2, 3} and a tail: the prefixes {0, 1} and {0, 1, 2, 3} both have cut 0
    src = [0, 1, 2, 3, 4, 5]
    dst = [1, 0, 3, 2, 5, 4]
    row_ptr = np.arange(7, dtype=np.int64)
    col = np.array(dst, dtype=np.int32)
    assert src == list(range(6))
    r = R.sweep_row(np.array([60, 50, 40, 30, 0, 0], dtype=np.uint64), row_ptr, col, 1)
    assert r["order"] == [0, 1, 2, 3] and r["cut"] == [1, 0, 1, 0] and r["vol"] == [1, 2, 3, 4]
    assert r["best"] == 2 and r["conductance"] == 0.0
    # cut / den 1/1 at the first prefix and 3/3 at the second
    row_ptr = np.array([0, 1, 3, 5, 6, 7, 8, 9], dtype=np.int64)
    col = np.array([2, 3, 4, 0, 1, 5, 6, 3, 4], dtype=np.int32)
    r = R.sweep_row(np.array([9, 8, 0, 0, 0, 0, 0], dtype=np.uint64), row_ptr, col, 1)
    assert r["cut"] == [1, 3] and r["vol"] == [1, 3] and r["best"] == 1 and r["conductance"] == 1.0


def test_generators_equal_brute_force():
    """every row / graph generator of sweep_ref.py the GPU shape tests use, at a size the brute force takes"""
    rng = np.random.Generator(np.random.PCG64(7200))
    row_ptr, col = _random_graph(rng, 120)
    deg = np.diff(row_ptr)
    # hubs first: degree descending, ties by id, full support
    row = R.hubs_first_row(row_ptr)
    full = R.sweep_row(row, row_ptr, col, 1)
    assert full["order"] == sorted(range(120), key=lambda v: (-int(deg[v]), v))
    _same(full, R.sweep_brute(row, row_ptr, col, 1))
    _same(R.sweep_row(row, row_ptr, col, 1, 17), R.sweep_brute(row, row_ptr, col, 1, 17))
    # the tie-heavy row and its cut-down copies
    row = R.tie_heavy_row(120, row_ptr, 7201)
    assert len(set(R.keys_in_order(row, row_ptr, R.sweep_row(row, row_ptr, col, 1)["order"]))) <= 5
    for length in (1, 40):
        cutdown = R.row_of_length(row, length)
        assert int((cutdown > 0).sum()) == length and (cutdown[cutdown > 0] == row[cutdown > 0]).all()
        _same(R.sweep_row(cutdown, row_ptr, col, 1), R.sweep_brute(cutdown, row_ptr, col, 1))
    # words at the edges of the key's range
    row, zero = R.edge_words_row(120, row_ptr, 7202, count=12)
    r = R.sweep_row(row, row_ptr, col, 1)
    _same(r, R.sweep_brute(row, row_ptr, col, 1))
    keys = R.keys_in_order(row, row_ptr, r["order"])
    assert keys[0] == FIX_ONE and deg[r["order"][0]] == 1
    assert r["order"][-zero.size:] == zero.tolist() and keys[-zero.size:] == [0] * zero.size and keys[-zero.size - 1] == 1
    above = {k for k in keys if k & 0xFFFFFFFF == 12345}
    below = {k for k in keys if k >> 33 == 9}
    assert len(above) >= 3 and len({k >> 33 for k in above}) == len(above) and len(below) >= 6 and len({k >> 32 for k in below}) == 1
    # ring, pairs, ring with chords and a hub
    for n, rp, cl, row in (R.ring_graph(9), R.ring_graph(12), R.pair_graph(5)):
        r = R.sweep_row(row, rp, cl, 1)
        assert r["order"] == list(range(n))
        _same(r, R.sweep_brute(row, rp, cl, 1))
    n, rp, cl = R.chord_ring_graph(n=90, chords=12, hub_deg=40, seed=7203)
    d = np.diff(rp)
    assert d[0] >= 42 and (d >= 2).all() and int(rp[-1]) == cl.size and all(cl[rp[u]:rp[u + 1]].tolist() == sorted(set(cl[rp[u]:rp[u + 1]].tolist())) for u in range(n))
    assert all((u + 1) % n in cl[rp[u]:rp[u + 1]] and (u - 1) % n in cl[rp[u]:rp[u + 1]] for u in range(n))
    row = R.hubs_first_row(rp)
    _same(R.sweep_row(row, rp, cl, 1), R.sweep_brute(row, rp, cl, 1))
    assert R.minimisers([3, 1, 1, 0], [1, 2, 4, 6], 6) == [1, 2] and R.minimisers([0], [0], 5) == []
    assert R.tied_boundaries([5, 5, 4, 4, 4, 3], 2) == (1, 2)


RING_TIES = {9: (3, 4), 513: (255, 256), 2049: (1023, 1024), 8193: (4095, 4096)}


def test_rings_and_pairs_have_tied_minimisers():
    """what tests/test_sweep_shapes_gpu.py relies on: two adjacent minimising prefixes either side of a lane, a wave, a scan
    step and position 4096; the twin takes the smaller"""
    for m, (a, b) in RING_TIES.items():
        n, rp, cl, row = R.ring_graph(m)
        r = R.sweep_row(row, rp, cl, 1)
        assert set(r["cut"][:-1]) == {2} and r["cut"][-1] == 0 and r["vol"] == [2 * (j + 1) for j in range(m)]
        assert R.minimisers(r["cut"], r["vol"], int(rp[-1])) == [a, b] and r["best"] == a + 1
    for m, unit in ((9, 4), (513, 64), (2049, 1024), (8193, 4096)):   # a lane's positions, a wave's lanes, a scan step, the tile
        assert RING_TIES[m][0] // unit + 1 == RING_TIES[m][1] // unit
    n, rp, cl, row = R.pair_graph(3000)
    r = R.sweep_row(row, rp, cl, 1)
    assert R.minimisers(r["cut"], r["vol"], int(rp[-1])) == list(range(1, 5999, 2)) and r["best"] == 2 and r["conductance"] == 0.0


def test_long_rows_have_the_ties_and_classes_the_gpu_tests_need(small_dangling):
    g = small_dangling
    nnz = int(g.row_ptr[-1])
    assert (g.deg == 0).any()
    mins = []
    for seed in R.TIE_SEEDS:
        row = R.tie_heavy_row(g.n, g.row_ptr, seed)
        r = R.sweep_row(row, g.row_ptr, g.col, 1)
        keys = R.keys_in_order(row, g.row_ptr, r["order"])
        assert r["len"] > 6 * 4096 and len(set(keys)) == 5
        tied = [R.tied_boundaries(keys, s) for s in (64, 1024, 4096)]
        print(seed, r["len"], tied)
        assert tied[1] == (24, 24) and tied[2] == (6, 6) and tied[0][0] >= tied[0][1] - 1
        if seed == R.TIE_SEEDS[0]:
            assert tied[0][0] == tied[0][1] >= 398
        mins.append(len(R.minimisers(r["cut"], r["vol"], nnz)))
    assert max(mins) >= 2   # a long row with equal conductances, too
    row = R.hubs_first_row(g.row_ptr)
    order = R.sweep_row(row, g.row_ptr, g.col, 1, 256)["order"]
    d = g.deg[order]
    assert (int((d >= 256).sum()), int(((d >= 64) & (d < 256)).sum())) == R.HUB_CLASSES


@pytest.mark.parametrize("L", R.SCAN_LENGTHS)
def test_scan_cases_plant_what_they_say(L):
    rng = np.random.Generator(np.random.PCG64(7300 + L))
    seen = 0
    for kind in R.SCAN_KINDS:
        for p, q in R.SCAN_PLACES.values():
            if q >= L:
                continue
            diff, vol, nnz, winner = R.scan_planted(rng, L, kind, p, q)
            ref = R.scan_ref(diff, vol, nnz)
            assert diff.dtype == np.int64 and vol.dtype == np.uint64 and len(diff) == len(vol) == L
            assert R.minimisers(ref["cut"], ref["vol"], nnz) == ([p, q] if kind == "tie" else [winner]) and ref["best"] == winner + 1
            a, b = (ref["cut"][p], ref["vol"][p]), (ref["cut"][q], ref["vol"][q])
            left, right = a[0] * b[1], b[0] * a[1]
            assert left >> 64 and right >> 64
            if kind == "tie":
                assert left == right and a != b
            elif kind.startswith("high"):
                assert left >> 64 == right >> 64 and left != right
            else:
                assert ((left & (2 ** 64 - 1)) < (right & (2 ** 64 - 1))) != (left < right)
            seen += 1
    assert seen == {1: 0, 4: 5, 5: 5, 1024: 15, 1025: 20, 5000: 25}[L]
    # the background alone: denominators from both sides of nnz / 2, none at the last prefix; and one with slack
    diff, vol, nnz = R.scan_plain(rng, L)
    ref = R.scan_ref(diff, vol, nnz)
    assert ref["edges"] == nnz and (ref["best"] == 0) == (L == 1)
    assert R.scan_ref(*R.scan_plain(rng, L, 12345))["best"] > 0
    # no prefix with a denominator
    ref = R.scan_ref(np.ones(L, np.int64), np.zeros(L, np.uint64), 77)
    assert (ref["best"], ref["cut_best"], ref["vol_best"], ref["den"], ref["edges"]) == (0, 0, 0, 0, 0) and ref["cut"] == list(range(1, L + 1))


def test_planted_block_is_recovered_on_twin_rows(oracle):
    n, row_ptr, col, block = R.planted_graph()
    assert n == 1999 and block.size == 300
    g = oracle.Graph(n, int(row_ptr[-1]), row_ptr, col)
    rmax, omega = oracle.fora_setting(g.n, g.m, 0.5)
    inside = set(block.tolist())
    rng = np.random.Generator(np.random.PCG64(7100))
    for s in rng.choice(block, size=4, replace=False):
        row, _, _ = oracle.twin_query(g, int(s), rmax, omega, seed=0x464F5241)
        for t in (0.0, 1.0 / n):
            r = R.sweep_row(row, row_ptr, col, R.thr_fix_of(t))
            got = set(r["order"][:r["best"]])
            jac = len(got & inside) / len(got | inside)
            print(f"source {int(s)} threshold {t:g}: best {r['best']} conductance {r['conductance']:.4f} jaccard {jac:.4f}")
            assert jac >= 0.9, (int(s), t, jac)


def test_c_abi_declares_exports_and_binds_the_sweep():
    hdr = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("fora_hip_sweep_batch", "fora_hip_sweep_fetch", "fora_hip_sweep_clear"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    assert "SWEEP CUT" in hdr
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    lib = capi.load()
    for name in ("fora_hip_sweep_batch", "fora_hip_sweep_fetch", "fora_hip_sweep_clear"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    # (fora_sweep_row and fora_sweep_stats against the header and the compiler: tests/test_capi_cpu.py)
    assert capi.STRUCTS["fora_sweep_row"] is capi.SweepRow and capi.STRUCTS["fora_sweep_stats"] is capi.SweepStats
    for meth in ("sweep", "sweep_fetch", "sweep_clear", "local_cluster"):
        assert callable(getattr(capi.Engine, meth))
    # NULL ctx: answered without touching the GPU
    assert lib.fora_hip_sweep_batch(None, None, 0, 0, 0.0, 0, None, None, None, None) == -1
    assert lib.fora_hip_sweep_fetch(None, None, None, None, 0) == -1
    assert lib.fora_hip_sweep_clear(None) == -1


def test_test_entry_points_are_in_the_test_library_only():
    """the TEST ENTRY POINTS of include/fora_hip.h: exported by libfora_hip_test.so, absent from the product library, from
    its symbol list and from the header's declarations"""
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    assert {"fora_hip_test_sweep_rows", "fora_hip_test_sweep_scan"} <= set(capi.TEST_SYMBOLS) and len(capi.TEST_SYMBOLS) == 5
    product, test = capi.load(), capi.load(capi.TEST_LIB)
    hdr = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    assert "TEST ENTRY POINTS" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in capi.TEST_SYMBOLS:
        assert hasattr(test, name) and not hasattr(product, name), name
        assert name not in capi.SYMBOLS and name not in code and name in hdr
    for name in capi.SYMBOLS:
        assert hasattr(test, name), name
    # NULL ctx: answered without touching the GPU
    assert test.fora_hip_test_sweep_rows(None, None, 0, 0.0, 0, None, None, None) == -1
    assert test.fora_hip_test_sweep_scan(None, None, None, 0, 0, None) == -1
    for meth in ("test_sweep_rows", "test_sweep_scan"):
        assert callable(getattr(capi.Engine, meth))


# ---- the plan of a sweep batch (fora_amd/csrc/fora_sweep_plan.h): tests/sweep_plan_check.cpp restates it by brute force and
# runs under the address and undefined-behaviour sanitizers; the sanitized code is that stand-alone program and nothing else
@pytest.fixture(scope="session")
def sweep_plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sweep_plan") / "sweep_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sweep_plan_check.cpp")], check=True)
    return exe


def _plan_check(exe, *args):
    r = subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    return r.stdout.split()


def test_sort_tile_of_the_option(sweep_plan_check):
    caps = [-1, 0, 1, 2, 3, 63, 64, 100, 4096, 5000]
    assert [int(x) for x in _plan_check(sweep_plan_check, "tile", *caps)] == [1, 1, 1, 2, 2, 32, 64, 64, 4096, 4096]


@pytest.mark.parametrize("T", [1, 2, 64, 4096])
def test_batch_plan_equals_brute_force(sweep_plan_check, T):
    """supports around every power of two up to 5 and around the tile, in one batch and split over several; profiles cut at
    1, at 3, not at all and above every support; rows placed through `at` with dangling rows between, and as r0 + i"""
    supports = sorted({0, 1, 2, 3, 4, 5, T - 1, T, T + 1, 2 * T, 2 * T + 1})
    nlive = len(supports)
    pow2 = lambda x: 0 if x == 0 else 1 << (x - 1).bit_length()
    with_dangling = ["d9"] + [str(s) for s in supports]
    for at in (2, 5, nlive + 2):      # first, between two rows of a batch, at a batch's edge for the 3 + rest split, last
        with_dangling.insert(at, "d9")
    with_dangling.append("d8")
    for rows in ("*" + ",".join(map(str, supports)), ",".join(with_dangling)):
        for batches in ([nlive], [1] * nlive, [3, nlive - 3], [nlive - 2, 1, 1]):
            for max_size in (0, 1, 3, 2 * T + 7):
                words = _plan_check(sweep_plan_check, "plan", T, max_size, rows, ",".join(map(str, batches)))
                assert words[-1] == "ok"
                f = {k: int(v) for k, v in (w.split("=") for w in words[:-1])}
                P = [pow2(s) for s in supports]
                assert f["live"] == nlive and f["maxP"] == max(P) and f["global_rows"] == sum(p > T for p in P)
                assert f["tiles"] == (0 if T == 1 else sum(-(-p // T) for p in P))
                assert f["words"] == 5 * nlive + 2 * f["tiles"] + 2 * f["global_rows"]
                held = sum(min(s, max_size) if max_size > 0 else s for s in supports)
                assert f["entries"] == held + (0 if rows[0] == "*" else 5)
