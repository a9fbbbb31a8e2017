"""BiPPR on CPU: the C ABI and the Engine declare the backward push and the BiPPR entry, and the two Python
restatements of the backward push (tests/bippr_ref.py: the fixed-point twin and the reference's f64 FIFO order) satisfy
the backward invariant against exact PPR.  The GPU runs are in test_bippr_gpu.py."""
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
