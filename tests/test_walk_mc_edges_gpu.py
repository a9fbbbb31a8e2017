"""k_walk_mc (fora_kernels.h) at its edges, through fora_hip_montecarlo_batch and fora_hip_bippr_batch: both
graph arms (the bit-packed copy and the plain CSR), walks longer than 512 and 1024 steps (the kernel's own copy of the
Philox counter), endpoints that overflow and wrap the 8 probes of the LDS table, fewer walks than lanes, waves and
workgroups can share out, and every node of a graph as a slot of one grid.

Every expected value comes from the CPU oracle (oracle.walk for the endpoints, oracle.walk_steps for the step counts) and
from restatements in plain Python of host arithmetic (walk weights, home slots, launch shape); none from a GPU call.  Every
case asserts from the oracle's walks alone that it runs what it claims to run, before the comparison that relies on it."""
import contextlib
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import bippr_ref as br
from test_baselines_gpu import FIX_ONE, SEED, _topk_of, mc_from_endpoints, mc_walks, twin_mc
from test_bippr_shapes_gpu import EPS, _check_bippr, _ends, _even_batch
from conftest import pick_sources

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAB_BITS, PROBES, PER_WG_MIN = 11, 8, 1 << 12  # fora_kernels.h / fora_hip.hip, asserted by test_source_constants
ARMS = pytest.mark.parametrize("no_compact", [0, 1], ids=["compact", "csr"])


def test_source_constants():
    """The cases below are built around these values; if the table or the launch changes they must be rebuilt."""
    ker = open(os.path.join(ROOT, "fora_amd", "csrc", "fora_kernels.h")).read()
    hip = open(os.path.join(ROOT, "fora_amd", "csrc", "fora_hip.hip")).read()
    assert re.search(r"constexpr int MC_TAB_BITS = %d;" % TAB_BITS, ker)
    assert re.search(r"constexpr int MC_PROBES = %d;" % PROBES, ker)
    assert re.search(r"uint32_t h = \(v \* 0x9E3779B1u\) >> \(32 - MC_TAB_BITS\);", ker)  # the home slot
    assert re.search(r"h = \(h \+ 1\) & \(MC_TAB - 1\);", ker)                            # linear probing, wrapping
    # launch_mc_walks: about eight workgroups per CU over the batch's slots, at least 4 Ki walk numbers each
    assert re.search(r"wgs = std::max<uint64_t>\(1, \(uint64_t\)c->prop\.multiProcessorCount \* 8 / \(uint64_t\)nb\);", hip)
    assert re.search(r"per_wg = std::min<uint64_t>\(1 << 16, std::max<uint64_t>\(1 << 12, \(j1 - j0 \+ wgs - 1\) / wgs\)\);", hip)
    assert PER_WG_MIN == 1 << 12 and int(_home(np.array([1]))[0]) == 0x9E3779B1 >> (32 - TAB_BITS)


def _home(v):
    """Home slot of endpoint v in the table of mc_tab_add: ((v * 0x9E3779B1) mod 2^32) >> 21."""
    return ((np.asarray(v, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - TAB_BITS)


def _launch_shape(cus, nb, W):
    """(per_wg, workgroups per slot) of launch_mc_walks for a batch of nb slots with W walks each (one launch)."""
    assert nb * W <= 1 << 28
    wgs = max(1, cus * 8 // nb)
    per_wg = min(1 << 16, max(PER_WG_MIN, -(-W // wgs)))
    return per_wg, -(-W // per_wg)


def _eps_for(n, W):
    """The epsilon at which montecarlo_setting gives omega = W - 0.5, W walks."""
    eps = math.sqrt(3 * math.log(2 * n) * n / (W - 0.5))
    assert mc_walks(n, eps)[1] == W
    return eps


@functools.lru_cache(maxsize=None)
def _walks(oracle, g, s, W, alpha):
    """(endpoints, steps) of walks j < W of source s, stream s, round 0 from the CPU oracle: what oracle.walk and
    oracle.walk_steps return, from one orc_walk call per walk with the arguments converted once (a case here needs up to
    340 000 walks).  (The cache takes the graph by identity and holds it.)"""
    orc_walk = oracle.lib().orc_walk
    n, rp, col = C.c_int32(g.n), g.row_ptr.ctypes.data_as(C.c_void_p), g.col.ctypes.data_as(C.c_void_p)
    seed, stream, rnd, start, a, nzh = C.c_uint64(SEED), C.c_uint32(s), C.c_uint32(0), C.c_int32(s), C.c_double(alpha), C.c_int(0)
    ends, steps = np.empty(W, dtype=np.int64), np.empty(W, dtype=np.int64)
    st = C.c_int64(0)
    pst = C.byref(st)
    for j in range(W):
        st.value = 0
        ends[j] = orc_walk(n, rp, col, seed, stream, rnd, start, C.c_uint64(j), a, nzh, pst)
        steps[j] = st.value
    for j in sorted({0, W // 2, W - 1}):  # the public wrappers agree
        assert ends[j] == oracle.walk(g, SEED, s, 0, s, j, alpha=alpha) and steps[j] == oracle.walk_steps(g, SEED, s, 0, s, j, alpha=alpha)
    ends.setflags(write=False)
    steps.setflags(write=False)
    return ends, steps


@contextlib.contextmanager
def _loaded(engine, g, no_compact, alpha=0.2):
    """The graph under `no_compact` (read by set_graph); options, batch, alpha and the graph's copies as they were after."""
    engine.reset_options()
    engine.set_batch(0)
    engine.set_option("no_compact", no_compact)
    try:
        engine.clear_index()
        engine.set_graph(g.n, g.m, g.row_ptr, g.col)
        engine.set_params(alpha=alpha, epsilon=0.5, seed=SEED)
        assert engine.get_option("no_compact") == no_compact
        yield
    finally:
        engine.reset_options()
        engine.set_batch(0)
        engine.set_graph(g.n, g.m, g.row_ptr, g.col)
        engine.set_params(alpha=0.2, epsilon=0.5, seed=SEED)


def _run_mc(engine, oracle, g, srcs, W, alpha=0.2, batch=0, eps=None):
    """One fora_hip_montecarlo_batch call of W walks per source (the graph is loaded): rows, sums, walk and step counters
    against the oracle.  Returns (slots per batch, raw rows)."""
    srcs = np.asarray(srcs, dtype=np.int32)
    eps = _eps_for(g.n, W) if eps is None else eps
    assert mc_walks(g.n, eps)[1] == W
    engine.set_batch(batch)
    try:
        engine.reset_timing()
        _, fix, _, _, st = engine.montecarlo(srcs, epsilon=eps)
        t = engine.timing()
        per = _even_batch(srcs.size, engine.get_batch())
    finally:
        engine.set_batch(0)
    steps_all = 0
    for i, s in enumerate(srcs.tolist()):
        ends, steps = _walks(oracle, g, s, W, alpha)
        want = mc_from_endpoints(g.n, ends)
        steps_all += int(steps.sum())
        bad = np.flatnonzero(fix[i] != want)
        assert bad.size == 0, (W, i, s, bad.size, bad[:8].tolist())
        assert int(fix[i].sum()) == FIX_ONE and st[i]["ppr_sum_fix"] == FIX_ONE and st[i]["n_walks"] == W, (W, i, s)
        assert st[i]["dangling_source"] == int(g.deg[s] == 0)
        if g.deg[s] == 0:  # the closed form: every walk ends on the source, none takes a step
            assert fix[i][s] == FIX_ONE and np.count_nonzero(fix[i]) == 1 and int(steps.sum()) == 0
    assert t["walks"] == W * srcs.size, (W, t["walks"])
    assert t["walk_steps"] == steps_all, (W, t["walk_steps"], steps_all)
    return per, fix


# ---------------------------------------------------------------------------------------------- the graphs
@functools.lru_cache(maxsize=None)
def _five(oracle):
    """0 <-> 1, 2 -> {0, 3}, 3 -> 4, 4 dangling: a walk from 2 may circle in the 2-cycle or come back from the dangling end."""
    src, dst = np.array([0, 1, 2, 2, 3], dtype=np.int32), np.array([1, 0, 0, 3, 4], dtype=np.int32)
    g = oracle.Graph.from_edges(5, src.size, src, dst)
    assert g.deg.tolist() == [1, 1, 2, 1, 0]
    return g


@functools.lru_cache(maxsize=None)
def _ring(oracle, n=300):
    """A directed ring of 300 nodes with a chord from every third node and a second from every tenth; three nodes dangle."""
    dang = (77, 150, 299)
    i = np.arange(n)
    a, b = i[i % 3 == 0], i[i % 10 == 0]
    src = np.concatenate([i, a, b])
    dst = np.concatenate([(i + 1) % n, (7 * a + 3) % n, (b * b + 1) % n])
    keep = ~np.isin(src, dang)
    g = oracle.Graph.from_edges(n, int(keep.sum()), src[keep].astype(np.int32), dst[keep].astype(np.int32))
    assert np.flatnonzero(g.deg == 0).tolist() == list(dang) and g.deg.max() == 3
    return g


@functools.lru_cache(maxsize=None)
def _star(oracle, leaves, n=24576):
    """Source 0 points to every leaf and every leaf points back; the other nodes have no edges."""
    leaves = np.asarray(leaves, dtype=np.int32)
    src = np.concatenate([np.zeros(leaves.size, dtype=np.int32), leaves])
    dst = np.concatenate([leaves, np.zeros(leaves.size, dtype=np.int32)])
    g = oracle.Graph.from_edges(n, src.size, src, dst)
    assert g.deg[0] == leaves.size and (g.deg[leaves] == 1).all() and int(g.deg.sum()) == 2 * leaves.size
    return g


# ---------------------------------------------------------------------------------------------- 1. both graph arms: BiPPR
def test_bippr_on_the_csr_arm(engine, oracle, tiny_dangling):
    """fora_hip_bippr_batch with the walks on the plain CSR.  _check_bippr builds its expected rows from the walks' endpoints:
    the first two sources' from the CPU oracle, the others' from fora_hip_walks.  Those endpoints are then shown equal to the
    oracle's, so every expected row is the one the oracle's walks give."""
    g = tiny_dangling
    alpha = 0.2
    srcs = np.concatenate([pick_sources(g, 5, 801), pick_sources(g, 1, 802, want_dangling=True)]).astype(np.int32)
    assert (g.deg[srcs] > 0).sum() == 5 and g.deg[srcs[5]] == 0 and np.unique(srcs).size == 6
    W = br.bippr_setting(g.n, g.m, EPS)[2]
    with _loaded(engine, g, 1, alpha):
        engine.reset_timing()
        _check_bippr(engine, oracle, g, srcs, alpha)
        t = engine.timing()
    steps_all = 0
    for s in srcs.tolist():
        ends, steps = _walks(oracle, g, s, W, alpha)
        used = _ends(engine, oracle, g, s, W, alpha, s in srcs[:2].tolist())  # (cached by _check_bippr: no call is made here)
        assert (used == ends).all(), s
        steps_all += int(steps.sum())
    assert t["walks"] == W * srcs.size and t["walk_steps"] == steps_all, (t["walks"], t["walk_steps"], steps_all)


# ---------------------------------------------------------------------------------------------- 2. long walks
@ARMS
def test_long_walks_change_counter_word_3(engine, oracle, tiny_dangling, no_compact):
    """alpha = 0.004: the kernel's own copy of the Philox counter has to move word 3 at step 512 and again at step 1024
    (s ^ ((t >> 9) * 0x9E3779B9)) and wrap the 8-bit step field of word 2, or the walks end elsewhere."""
    g = tiny_dangling
    alpha, eps = 0.004, 3.0
    W = mc_walks(g.n, eps)[1]
    assert W == 5530
    live = int(pick_sources(g, 1, 811)[0])
    dang = int(pick_sources(g, 1, 812, want_dangling=True)[0])
    assert g.deg[live] > 0 and g.deg[dang] == 0
    ends, steps = _walks(oracle, g, live, W, alpha)
    assert (steps > 512).sum() >= 100 and (steps > 1024).sum() >= 10, ((steps > 512).sum(), (steps > 1024).sum())
    with _loaded(engine, g, no_compact, alpha):
        _run_mc(engine, oracle, g, [live, dang], W, alpha, eps=eps)


# ---------------------------------------------------------------------------------------------- 3. probe overflow and wrap-around
def _blocks(ends, per_wg):
    return [ends[lo:lo + per_wg] for lo in range(0, ends.size, per_wg)]


@ARMS
@pytest.mark.parametrize("H", [1000, 2045])
def test_table_overflow_and_wrap(engine, oracle, H, no_compact):
    """More distinct endpoints share home slot H than a key has probes: in every workgroup at least one add finds no entry
    and goes to HBM directly.  H = 2045: the probes run 2045, 2046, 2047, 0, 1, ..."""
    test_source_constants()
    n, W = 24576, 12288
    home = _home(np.arange(n)).astype(np.int64)
    per_slot = np.bincount(home, minlength=1 << TAB_BITS)
    assert per_slot.size == 1 << TAB_BITS and 11 <= per_slot.min() and per_slot.max() <= 14
    ids = np.flatnonzero(home == H)
    assert ids.size == {1000: 11, 2045: 12}[H] and ids.size > PROBES and 0 not in ids
    if H == 2045:
        assert H + PROBES > 1 << TAB_BITS and ids.size > (1 << TAB_BITS) - H  # some key's entry lies past the table's end
    g = _star(oracle, tuple(ids.tolist()))
    per_wg, X = _launch_shape(engine.device_info()[1], 1, W)
    assert (per_wg, X) == (4096, 3)
    ends, _ = _walks(oracle, g, 0, W, 0.2)
    for blk in _blocks(ends, per_wg):  # every workgroup meets every colliding id: more keys than probes (pigeonhole)
        assert blk.size == per_wg and np.isin(ids, blk).all() and np.setdiff1d(blk, ids).tolist() == [0]
    with _loaded(engine, g, no_compact):
        _run_mc(engine, oracle, g, [0], W)


@ARMS
def test_table_under_high_load(engine, oracle, no_compact):
    """About 1570 distinct endpoints per workgroup in a table of 2048: long probe chains, full ones among them."""
    test_source_constants()
    n, W = 24576, 12288
    g = _star(oracle, tuple(range(1, 6001)))
    per_wg, X = _launch_shape(engine.device_info()[1], 1, W)
    assert (per_wg, X) == (4096, 3)
    ends, _ = _walks(oracle, g, 0, W, 0.2)
    for blk in _blocks(ends, per_wg):
        assert np.unique(blk[blk != 0]).size >= 1400
    with _loaded(engine, g, no_compact):
        _run_mc(engine, oracle, g, [0], W)


# ---------------------------------------------------------------------------------------------- 4. few walks
@ARMS
@pytest.mark.parametrize("W", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257])
def test_fewer_walks_than_lanes_and_waves(engine, oracle, W, no_compact):
    """W < 4: some waves of the workgroup have no walk (lo + (span * wid >> 2)); W < 64 .. 256: the first refill hands out
    fewer walks than there are idle lanes.  W = 4: wrem = 0; W = 3: wrem = 1; W = 5: wrem = W - 1."""
    assert FIX_ONE % 4 == 0 and FIX_ONE % 3 == 1 and FIX_ONE % 5 == 4
    g = _five(oracle)
    assert _launch_shape(engine.device_info()[1], 2, W) == (4096, 1)
    with _loaded(engine, g, no_compact):
        _run_mc(engine, oracle, g, [2, 4], W)


@ARMS
@pytest.mark.parametrize("W", [4095, 4096, 4097])
def test_walks_around_one_workgroup(engine, oracle, W, no_compact):
    """per_wg = 4096: one workgroup short of a walk, exactly full, and a second workgroup that runs a single walk."""
    g = _ring(oracle)
    per_wg, X = _launch_shape(engine.device_info()[1], 2, W)
    assert per_wg == 4096 and X == (2 if W == 4097 else 1) and W - (X - 1) * per_wg == {4095: 4095, 4096: 4096, 4097: 1}[W]
    with _loaded(engine, g, no_compact):
        _run_mc(engine, oracle, g, [0, 150], W)


# ---------------------------------------------------------------------------------------------- 5. many slots in one grid
@ARMS
@pytest.mark.parametrize("batch", [0, 7])
def test_every_node_a_source(engine, oracle, batch, no_compact):
    """300 slots (three of them dangling) in one call: one grid of many slots, or 43 grids of 7 and 6."""
    g = _ring(oracle)
    W = 533
    srcs = np.arange(g.n, dtype=np.int32)
    with _loaded(engine, g, no_compact):
        per, _ = _run_mc(engine, oracle, g, srcs, W, batch=batch)
    if batch:
        assert per == 7 and g.n % per == 6
    else:
        assert per > 7
    assert _launch_shape(engine.device_info()[1], per, W) == (4096, 1)


@ARMS
def test_topk_of_tied_integer_weights(engine, oracle, no_compact):
    """533 walks: a row's entries are small multiples of one weight and tie heavily, also inside the first 20."""
    g = _ring(oracle)
    W, k = 533, 20
    srcs = np.array([0, 150, 7, 299, 160], dtype=np.int32)
    tied = 0
    for s in srcs.tolist():
        want = twin_mc(oracle, g, s, W)
        assert (want == mc_from_endpoints(g.n, _walks(oracle, g, s, W, 0.2)[0])).all()
        _, sc = _topk_of(want, k)
        tied += int((np.diff(sc[sc > 0]) == 0).sum())
    assert tied >= 10
    with _loaded(engine, g, no_compact):
        _, fix, ids, sc, _ = engine.montecarlo(srcs, epsilon=_eps_for(g.n, W), k=k)
    for i, s in enumerate(srcs.tolist()):
        assert (fix[i] == twin_mc(oracle, g, s, W)).all(), s
        want_ids, want_sc = _topk_of(fix[i], k)
        assert (ids[i] == want_ids).all() and (sc[i] == want_sc).all(), s
    assert ids[1][0] == 150 and sc[1][0] == 1.0 and (sc[1][1:] == 0).all() and (ids[1][1:] == 0).all()  # the dangling source: padded
