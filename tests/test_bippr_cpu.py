"""BiPPR on CPU: the C ABI and the Engine declare the backward push and the BiPPR entry, and the two Python
restatements of the backward push (tests/bippr_ref.py: the fixed-point twin and the reference's f64 FIFO order) satisfy
the backward invariant against exact PPR, at several depths and alphas and with dangling nodes; the pop rule on a residue
that equals the threshold.  The GPU runs are in test_bippr_gpu.py and test_bippr_shapes_gpu.py."""
import math
import os

import numpy as np
import pytest

import bippr_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = 0.2


def test_capi_declares_bippr_and_bwdpush():
    from fora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    for name in ("fora_hip_bippr_batch", "fora_hip_bwdpush_batch"):
        assert name in capi.SYMBOLS and f"int {name}(" in hdr
    assert "FORA_BWD_FIX_ONE (1ULL << 60)" in hdr and "fora_bwd_stats;" in hdr
    assert hasattr(capi.Engine, "bippr") and hasattr(capi.Engine, "bwdpush")
    assert [f for f, _ in capi.BwdStats._fields_] == ["targets", "pops", "relax", "entries", "global_targets", "levels",
                                                      "chunks", "bwd_ms", "walk_ms", "combine_ms"]


def test_bippr_setting_operand_order():
    n, m, eps, scale = 2000, 16000, 0.5, 1.7
    delta = pfail = 1.0 / n
    rmax = eps * math.sqrt(m * 1.0 * delta / 3.0 / math.log(2.0 / pfail))
    rmax *= scale
    omega = rmax * 3 * math.log(2.0 / pfail) / delta / eps / eps
    assert br.bippr_setting(n, m, eps, scale) == (rmax, omega, math.ceil(omega))
    r1, o1, w1 = br.bippr_setting(n, m, eps)
    assert abs(r1 - 0.28351174517377914) < 1e-15 and w1 == 56436


@pytest.fixture(scope="module")
def exact_pi(tiny):
    """Pi = alpha (I - (1 - alpha) P)^-1 of the dangling-free tiny graph, P[u, v] = (u -> v edges) / outdeg(u)."""
    g = tiny
    deg = np.diff(g.row_ptr)
    assert (deg > 0).all()
    P = np.zeros((g.n, g.n))
    src = np.repeat(np.arange(g.n), deg)
    np.add.at(P, (src, g.col[:src.size]), 1.0 / deg[src])
    return ALPHA * np.linalg.solve(np.eye(g.n) - (1 - ALPHA) * P, np.eye(g.n))


def test_twin_and_fifo_leave_residues_under_rmax_and_keep_the_invariant(tiny, exact_pi):
    g = tiny
    rmax = br.bippr_setting(g.n, g.m, 0.5)[0]
    Pi = exact_pi
    pops = relax = entries = levels = 0
    for kind in ("twin", "fifo"):
        worst = 0.0
        for t in range(g.n):
            if kind == "twin":
                p, r, po, re, lv = br.twin_bwd_push_sparse(g, t, rmax, ALPHA)
                pops, relax, entries, levels = pops + po, relax + re, entries + br.entries_of(p, r), max(levels, lv)
                rsv = np.zeros(g.n)
                res = np.zeros(g.n)
                for v, x in p.items():
                    rsv[v] = math.ldexp(x, -60)
                for v, x in r.items():
                    res[v] = math.ldexp(x, -60)
                assert max(r.values()) <= math.floor(math.ldexp(rmax, 60))
            else:
                rsv, res = br.fifo_bwd_push(g, t, rmax, ALPHA)
                assert res.max() <= rmax
            # pi(s, t) = p_t[s] + sum_v pi(s, v) r_t[v] for every s
            worst = max(worst, np.abs(Pi[:, t] - rsv - Pi @ res).max())
        assert worst <= 1e-12, (kind, worst)
    # the figures the issue's restatement gave for the tiny graph at eps = 0.5
    assert (pops, relax, entries) == (3963, 19415, 21216) and levels <= 6


def test_bippr_twin_rmax_over_one_is_the_walk_slab_over_four(tiny):
    g = tiny
    rng = np.random.default_rng(5)
    ends = rng.integers(0, g.n, size=1000)
    rmax = 1.25
    out = br.twin_bippr(g, 3, rmax, 1000, ends, ALPHA)
    assert (out == br.mc_slab(g.n, ends) // np.uint64(4)).all()


def _exact_pi(g, alpha):
    """Pi = alpha (I - (1 - alpha) P)^-1, P[u, v] = (u -> v edges) / outdeg(u) and a zero row for a dangling u."""
    deg = np.diff(g.row_ptr)
    P = np.zeros((g.n, g.n))
    src = np.repeat(np.arange(g.n), deg)
    np.add.at(P, (src, g.col[:src.size]), 1.0 / deg[src])
    return alpha * np.linalg.solve(np.eye(g.n) - (1 - alpha) * P, np.eye(g.n))


@pytest.mark.parametrize("alpha", [0.05, 0.2, 0.5])
@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling"])
def test_backward_invariant_deep_pushes(request, gname, alpha):
    """Pi[:, t] = p_t + Pi r_t is linear algebra: it holds for any P, with or without zero rows, after any number of
    pops.  The fixed-point twin floors once per pop (the keep) and once per relaxation (the increment), and a lost unit
    of 2^-60 weighs at most 1 in the identity (the entries of Pi are <= 1): a defect of at most (pops + relax) * 2^-60.
    On top of that comes the rounding of the f64 check itself (the solve, Pi @ r); that term is measured, not guessed:
    it is the defect of the f64 FIFO restatement on the same target, with a margin of 4.
    The 20 targets of a case include the node of largest in-degree, whose pushes are the longest; that is why the figures
    are larger than a random sample's.  Measured on these 20 targets per case: twin <= 3.1e-15, FIFO <= 3.1e-16, (pops + relax) * 2^-60 from 8.7e-19 (a
    target without in-edges) to 1.6e-12; the twin's defect is at most 0.25 of the bound.  At alpha 0.5, rmax 1e-2 the
    twin's 3.0e-16 exceeds the fixed-point term of some targets: the float term is needed."""
    g = request.getfixturevalue(gname)
    Pi = _exact_pi(g, alpha)
    indeg = np.bincount(g.col, minlength=g.n)
    rng = np.random.Generator(np.random.PCG64(77))
    targets = np.unique(np.concatenate([[int(indeg.argmax())], rng.choice(g.n, 19, replace=False)]))
    deepest = 0
    for rmax in (1e-2, 1e-4):
        thr = math.floor(math.ldexp(rmax, 60))
        for t in targets.tolist():
            p, r, pops, relax, levels = br.twin_bwd_push_sparse(g, t, rmax, alpha)
            assert max(r.values()) <= thr and br.support_of(r) >= set(p) and t in br.support_of(r)
            rsv = np.zeros(g.n)
            res = np.zeros(g.n)
            for v, x in p.items():
                rsv[v] = math.ldexp(x, -60)
            for v, x in r.items():
                res[v] = math.ldexp(x, -60)
            twin = np.abs(Pi[:, t] - rsv - Pi @ res).max()
            f_rsv, f_res = br.fifo_bwd_push(g, t, rmax, alpha)
            assert f_res.max() <= rmax
            fifo = np.abs(Pi[:, t] - f_rsv - Pi @ f_res).max()
            bound = math.ldexp(pops + relax, -60) + 4 * fifo
            assert twin <= bound, (gname, alpha, rmax, t, twin, fifo, pops, relax)
            deepest = max(deepest, levels)
    assert deepest > 6  # past the 6 levels of BiPPR's own rmax on these graphs


@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling"])
def test_twin_equals_its_plain_restatement(request, gname):
    """twin_bwd_push_sparse looks only at the nodes a level added to; the plain scan of every residue must give the same
    dicts (keys included: they are the support), counters and levels, shallow and deep."""
    g = request.getfixturevalue(gname)
    indeg = np.bincount(g.col, minlength=g.n)
    rng = np.random.Generator(np.random.PCG64(78))
    targets = [int(indeg.argmax()), int(np.flatnonzero(indeg == 0)[0])] + rng.choice(g.n, 6, replace=False).tolist()
    for alpha, rmax in ((0.2, 0.2835), (0.2, 1e-3), (0.05, 1e-3), (0.5, 1e-4), (0.85, 1e-4), (0.5, 1.0)):
        for t in targets:
            assert br.twin_bwd_push_sparse(g, t, rmax, alpha) == br.twin_bwd_push_scan(g, t, rmax, alpha), (alpha, rmax, t)


def test_support_helpers(tiny_dangling):
    g = tiny_dangling
    indeg = np.bincount(g.col, minlength=g.n)
    lone = int(np.flatnonzero(indeg == 0)[0])
    p, r, pops, relax, levels = br.twin_bwd_push_sparse(g, lone, 1e-3, ALPHA)
    assert br.support_of(r) == {lone} and (pops, relax, levels) == (1, 0, 1) and r[lone] == 0
    hub = int(indeg.argmax())
    _, r, _, _, _ = br.twin_bwd_push_sparse(g, hub, 0.9, ALPHA)  # one pop: the hub and its distinct in-neighbours
    rin_ptr, rin = br.reverse_csr(g)
    assert br.support_of(r) == {hub} | set(rin[rin_ptr[hub]:rin_ptr[hub + 1]].tolist())
    assert br.targets_over_cap([1, 5, 5, 9], 5) == 1 and br.targets_over_cap([1, 5, 5, 9], 4) == 3
    assert br.targets_over_cap([1, 5], 0) == 2
    s = br.slot_of(np.arange(5000))
    assert s.max() == 2047 and int(br.slot_of(1)) == 0x9E3779B1 >> 21 and int(br.slot_of(3)) == ((3 * 0x9E3779B1) & 0xFFFFFFFF) >> 21


def test_pop_rule_on_the_threshold(oracle):
    """pop iff r > floor(rmax * 2^60): a residue that equals the threshold stays, one ulp of rmax less and it pops."""
    n, src, dst, t, u = br.threshold_graph()
    g = oracle.Graph.from_edges(n, src.size, src, dst)
    alpha = 0.5
    assert int(math.ldexp(alpha, 62)) == 1 << 61
    # the neighbour: exactly 2^58 = 0.25 * 2^60
    p, r, pops, relax, levels = br.twin_bwd_push_sparse(g, t, 0.25, alpha)
    assert math.floor(math.ldexp(0.25, 60)) == 1 << 58
    assert (p, r, pops, relax, levels) == ({t: 1 << 59}, {t: 0, u: 1 << 58}, 1, 1, 1)
    below = math.nextafter(0.25, 0)
    assert math.floor(math.ldexp(below, 60)) == (1 << 58) - 32
    p, r, pops, relax, levels = br.twin_bwd_push_sparse(g, t, below, alpha)
    assert (p, r, pops, relax, levels) == ({t: 1 << 59, u: 1 << 57}, {t: 0, u: 0, 3: 1 << 57}, 2, 2, 2)
    # the target itself: exactly 2^60
    p, r, pops, relax, levels = br.twin_bwd_push_sparse(g, t, 1.0, alpha)
    assert (p, r, pops, relax, levels) == ({}, {t: 1 << 60}, 0, 0, 0)
    p, r, pops, relax, levels = br.twin_bwd_push_sparse(g, t, math.nextafter(1.0, 0), alpha)
    assert (p, r, pops, relax, levels) == ({t: 1 << 59}, {t: 0, u: 1 << 58}, 1, 1, 1)


def test_topk_of_order_ties_and_padding():
    fix = np.array([5, 0, 9, 5, 0, 9, 1], dtype=np.uint64)
    ids, sc = br.topk_of(fix, 4)
    assert ids.tolist() == [2, 5, 0, 3] and sc.tolist() == [math.ldexp(9, -60)] * 2 + [math.ldexp(5, -60)] * 2
    ids, sc = br.topk_of(fix, 7)
    assert ids.tolist() == [2, 5, 0, 3, 6, 0, 0] and sc[5:].tolist() == [0.0, 0.0]
