"""--algo montecarlo / fwdpush on the GPU (fora_hip_montecarlo_batch / fora_hip_fwdpush_batch), against CPU twins built
from the oracle's primitives: orc_walk for the Monte-Carlo walks, orc_twin_push for the push, power iteration for the
error bound."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import pick_sources
from test_cli import _write_dataset

pytestmark = pytest.mark.gpu
SEED = 0x464F5241
FIX_ONE = 1 << 62
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mc_walks(n, eps):
    """montecarlo_setting (algo.h:477-483) in the reference's operand order, and W = #{i >= 0 : i < omega}."""
    delta = pfail = 1.0 / n
    omega = 3 * math.log(2 / pfail) / eps / eps / delta
    return omega, math.ceil(omega)


def fwdpush_rmax(n, m, eps, rmax_scale=1.0):
    delta = 1.0 / n
    return rmax_scale * delta * eps * n / m  # fwdpush_setting, algo.h:485-496


def mc_from_endpoints(n, ends):
    """ppr of walks j = 0 .. W-1 ending at ends[j]: walk j carries floor(2^62 / W) + (j < 2^62 mod W) units."""
    W = ends.size
    base, rem = FIX_ONE // W, FIX_ONE % W
    return (np.bincount(ends, minlength=n).astype(np.uint64) * np.uint64(base)
            + np.bincount(ends[:rem], minlength=n).astype(np.uint64))


def twin_mc(oracle, g, s, W):
    ends = np.array([oracle.walk(g, SEED, s, 0, s, j) for j in range(W)], dtype=np.int64)
    return mc_from_endpoints(g.n, ends)


def _load(engine, g, eps=0.5):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(epsilon=eps, seed=SEED)
    return engine.get_params()


def _topk_of(fix, k):
    """score descending, ties id ascending, padded with (0, 0.0)"""
    nz = np.flatnonzero(fix)
    order = np.array(sorted(nz.tolist(), key=lambda v: (-int(fix[v]), v)), dtype=np.int64)[:k]
    ids = np.zeros(k, dtype=np.int32)
    sc = np.zeros(k, dtype=np.float64)
    ids[:order.size] = order
    sc[:order.size] = [math.ldexp(int(fix[v]), -62) for v in order]
    return ids, sc


@pytest.mark.parametrize("batch", [1, 0])
def test_montecarlo_bit_exact_vs_twin(engine, oracle, tiny_dangling, batch):
    g = tiny_dangling
    eps = 1.0
    _load(engine, g)
    omega, W = mc_walks(g.n, eps)
    assert 1e4 <= W <= 2e5
    dang = pick_sources(g, 1, 301, want_dangling=True)
    live = pick_sources(g, 3, 302)
    srcs = np.concatenate([dang, live]).astype(np.int32)
    engine.set_batch(batch)
    try:
        _, fix, _, _, st = engine.montecarlo(srcs, epsilon=eps)
    finally:
        engine.set_batch(0)
    hits_dangling = False
    for i, s in enumerate(srcs):
        want = twin_mc(oracle, g, int(s), W)
        assert (fix[i] == want).all(), (int(s), int(np.flatnonzero(fix[i] != want).size))
        assert int(fix[i].sum()) == FIX_ONE and st[i]["ppr_sum_fix"] == FIX_ONE and st[i]["n_walks"] == W
        assert st[i]["dangling_source"] == int(g.deg[s] == 0)
        if g.deg[s] > 0:
            hits_dangling |= bool(((fix[i] > 0) & (g.deg == 0)).any())  # walks that reached a dangling node (and jumped back)
    assert g.deg[srcs[0]] == 0 and fix[0][srcs[0]] == FIX_ONE
    assert hits_dangling


def test_montecarlo_webstanford_size(engine, oracle):
    """ws-sized R-MAT (n = 281 904): ~44.8 M walks per source."""
    from fora_amd import synth
    n, m, rp, col = synth.preset("webstanford")
    engine.clear_index()
    engine.set_graph(n, m, rp, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    omega, W = mc_walks(n, 0.5)
    assert 44e6 < W < 46e6
    srcs = synth.query_set(n, 2, 5)
    engine.reset_timing()
    ppr, fix, _, _, st = engine.montecarlo(srcs, epsilon=0.5, want_ppr=True)
    t = engine.timing()
    assert t["walks"] == 2 * W and t["walk_steps"] > 2 * W and t["walk_ms"] > 0
    exact, _, _, _ = engine.power_iteration(srcs)
    for i, s in enumerate(srcs):
        s = int(s)
        assert st[i]["n_walks"] == W and st[i]["ppr_sum_fix"] == FIX_ONE and int(fix[i].sum()) == FIX_ONE
        ends = engine.walks(s, 0, np.full(W, s, dtype=np.int32), np.arange(W, dtype=np.uint64)).astype(np.int64)
        assert (fix[i] == mc_from_endpoints(n, ends)).all()
        big = exact[i] >= 1.0 / n
        assert (np.abs(ppr[i] - exact[i])[big] <= 0.5 * exact[i][big]).all()


def test_montecarlo_second_walk_launch(engine):
    """Eight ws-sized sources in one batch: 8 W walks are more than one launch of launch_mc_walks runs (MC_LAUNCH_WALKS =
    2^28 over all slots of the batch), so every slot's walks j >= 2^28 / 8 come from a second launch (j0 > 0)."""
    import re
    from fora_amd import synth
    src = open(os.path.join(ROOT, "fora_amd", "csrc", "fora_hip.hip")).read()
    assert re.search(r"MC_LAUNCH_WALKS\s*=\s*1ull\s*<<\s*28\b", src)  # the launch limit the arithmetic below is about
    n, m, rp, col = synth.preset("webstanford")
    engine.clear_index()
    engine.set_graph(n, m, rp, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    omega, W = mc_walks(n, 0.5)
    nb = 8
    assert nb * W > 1 << 28 and (1 << 28) // nb < W <= 2 * ((1 << 28) // nb)  # two launches
    srcs = synth.query_set(n, nb, 11)
    engine.set_batch(nb)
    try:
        _, fix, _, _, st = engine.montecarlo(srcs, epsilon=0.5)
        assert engine.get_batch() >= nb  # all eight sources in one batch
    finally:
        engine.set_batch(0)
    js = np.arange(W, dtype=np.uint64)
    starts = np.zeros(W, dtype=np.int32)
    for i, s in enumerate(srcs):
        s = int(s)
        assert st[i]["n_walks"] == W and st[i]["ppr_sum_fix"] == FIX_ONE and int(fix[i].sum()) == FIX_ONE
        starts.fill(s)
        ends = engine.walks(s, 0, starts, js)
        assert (fix[i] == mc_from_endpoints(n, ends)).all(), (i, s)


@pytest.mark.parametrize("layout", ["team", "bucketed", "wide"])
@pytest.mark.parametrize("gname", ["tiny_dangling", "small"])
def test_fwdpush_bit_exact_vs_twin(engine, oracle, request, gname, layout):
    g = request.getfixturevalue(gname)
    if layout != "team":
        engine.set_option("team", 0)
        engine.set_option("tail", 0)
    if layout == "wide":
        engine.set_option("force_wide", 1)
    try:
        _load(engine, g)
        rmax = fwdpush_rmax(g.n, g.m, 0.5, 2.0)
        srcs = np.concatenate([pick_sources(g, 5, 311), pick_sources(g, 1, 312, want_dangling=True)])
        ppr, rsv, res, _, _, st = engine.fwdpush(srcs, epsilon=0.5, rmax_scale=2.0, want_ppr=True)
        thr = math.ceil(math.ldexp(rmax, 62))
        for i, s in enumerate(srcs):
            t = oracle.twin_push(g, int(s), rmax)
            assert (rsv[i] == t["reserve"]).all() and (res[i] == t["residue"]).all()
            assert st[i]["rmax_used"] == rmax
            assert st[i]["pops"] == t["pops"] and st[i]["relax"] == t["relax"] and st[i]["levels"] == t["levels"]
            assert st[i]["rsum_fix"] == t["rsum_fix"] and st[i]["ppr_sum_fix"] == FIX_ONE - t["rsum_fix"]
            assert int(rsv[i].sum()) + int(res[i].sum()) == FIX_ONE
            live = res[i] > 0   # exit: every residue below rmax * outdeg (a dangling node keeps none)
            assert (res[i][live].astype(object) < np.array([thr * int(d) for d in g.deg[live]], dtype=object)).all()
            assert (ppr[i] == np.ldexp(rsv[i].astype(np.float64), -62)).all()
    finally:
        engine.reset_options()


def test_topk_matches_dense_output(engine, oracle, tiny_dangling):
    g = tiny_dangling
    _load(engine, g)
    dang = pick_sources(g, 1, 321, want_dangling=True)
    srcs = np.concatenate([pick_sources(g, 3, 322), dang]).astype(np.int32)
    k = 40
    _, fix, ids, sc, _ = engine.montecarlo(srcs, epsilon=1.0, k=k)
    _, rsv, _, ids2, sc2, _ = engine.fwdpush(srcs, epsilon=0.5, rmax_scale=50.0, k=k)
    for i in range(srcs.size):
        for f, a, b in ((fix[i], ids[i], sc[i]), (rsv[i], ids2[i], sc2[i])):
            wi, ws = _topk_of(f, k)
            assert (a == wi).all() and (b == ws).all()
    # padding: a dangling source has one non-zero entry; the large rmax leaves fewer than k reserve entries
    assert ids[-1][0] == dang[0] and sc[-1][0] == 1.0 and (sc[-1][1:] == 0).all() and (ids[-1][1:] == 0).all()
    assert (sc2 == 0).any()


def test_fora_not_disturbed(engine, oracle, small):
    g = small
    params = _load(engine, g)
    srcs = pick_sources(g, 4, 331)
    a_ppr, a_res, _ = engine.query_fix(srcs)
    engine.montecarlo(srcs, epsilon=0.7)
    assert engine.get_params() == params
    engine.fwdpush(srcs, epsilon=0.5, rmax_scale=3.0, k=10)
    assert engine.get_params() == params
    b_ppr, b_res, _ = engine.query_fix(srcs)
    assert (a_ppr == b_ppr).all() and (a_res == b_res).all()
    ids, sc, _ = engine.topk(srcs, 10)
    want, _, _, _ = oracle.twin_topk_query(g, int(srcs[0]), 10, 0.5, seed=SEED)
    assert (ids[0] == want).all()


def test_argument_errors(engine, tiny):
    from fora_amd import ForaError
    g = tiny
    params = _load(engine, g)
    good = np.array([1, 2], dtype=np.int32)
    bad_calls = [
        lambda: engine.montecarlo(np.array([g.n], dtype=np.int32)),
        lambda: engine.montecarlo(np.array([-1], dtype=np.int32)),
        lambda: engine.montecarlo(good, epsilon=0.0),
        lambda: engine.montecarlo(good, epsilon=-1.0),
        lambda: engine.fwdpush(np.array([g.n], dtype=np.int32)),
        lambda: engine.fwdpush(good, epsilon=0.0),
        lambda: engine.fwdpush(good, k=2000),
    ]
    for call in bad_calls:
        with pytest.raises(ForaError) as e:
            call()
        assert e.value.code == -1
    import ctypes as C
    lib, ctx = engine._lib, engine._ctx
    assert lib.fora_hip_montecarlo_batch(ctx, good.ctypes.data, C.c_int(-1), C.c_double(0.5), None, None, C.c_int(0), None, None,
                                         None) == -1
    assert lib.fora_hip_fwdpush_batch(ctx, good.ctypes.data, C.c_int(2), C.c_double(0.5), C.c_double(1.0), None, None, None,
                                      C.c_int(-1), None, None, None) == -1
    assert engine.get_params() == params
    ppr, _, st = engine.query_fix(good)
    assert all(s["ppr_sum_fix"] == FIX_ONE for s in st)


def test_cli_end_to_end(oracle, small, tmp_path):
    import __graft_entry__
    __graft_entry__.build()
    cli = os.path.join(ROOT, "fora_amd", "bin", "fora")
    g = small
    queries = pick_sources(g, 6, 341)
    _write_dataset(str(tmp_path / "data" / "g32k"), g, queries)
    common = ["--prefix", str(tmp_path / "data") + "/", "--dataset", "g32k", "--epsilon", "0.5",
              "--result_dir", str(tmp_path / "res")]
    run = lambda *a: subprocess.run([cli, *a, *common], capture_output=True, text=True, timeout=900)
    r = run("gen-exact-topk", "--k", "20", "--query_size", "6")
    assert r.returncode == 0, r.stderr
    keys = None
    for algo, slot in (("montecarlo", "1"), ("fwdpush", "5")):
        r = run("query", "--algo", algo, "--query_size", "4", "--gpus", "2", "--oversubscribe")
        assert r.returncode == 0, r.stderr
        assert "4. source node:%d" % queries[3] in r.stdout and "Total cost (s):" in r.stdout
        j = json.load(open(tmp_path / "res" / "execution" / f"g32k.query.{algo}.without_idx.k-500.rmax-1.000000.json"))
        assert j["config"]["algo"] == algo and slot in j["timer"]
        keys = keys or (set(j["config"]), set(j["result"]))
        assert (set(j["config"]), set(j["result"])) == keys
        if algo == "montecarlo":
            omega, W = mc_walks(g.n, 0.5)
            assert float(j["config"]["omega"]) == omega and float(j["result"]["total number of rand-walks"]) == 4 * W
            assert "6" in j["timer"]
        else:
            assert float(j["config"]["rmax"]) == fwdpush_rmax(g.n, g.m, 0.5)
        r = run("topk", "--algo", algo, "--k", "20", "--query_size", "5")
        assert r.returncode == 0, r.stderr
        assert "Average top-K Precision:" in r.stdout and "Precision:" in r.stdout
        j = json.load(open(tmp_path / "res" / "execution" / f"g32k.topk.{algo}.without_idx.k-20.rmax-1.000000.json"))
        assert 0.5 < float(j["result"]["topk precision"]) <= 1.0
        lines = open(tmp_path / "res" / "g32k.topk.k-20.txt").read().strip().split("\n")
        assert len(lines) == 5 and int(lines[0].split()[0]) == queries[0]
        r = run("batch-topk", "--algo", algo, "--k", "20", "--query_size", "5")
        assert r.returncode == 0, r.stderr
        tab = r.stdout.split("\n" + algo + "\n")[-1].split("\n")   # display_precision_for_dif_k, algo.h:676-692
        assert tab[0].split() == ["4", "8", "12", "16", "20"] and tab[1] == "Precision:" and tab[3] == "Recall:"
        assert len(tab[2].split()) == 5 and all(0.0 < float(x) <= 1.0 for x in tab[2].split())
