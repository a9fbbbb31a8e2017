"""BiPPR in Python (test helper): bippr_setting (algo.h:442-447), the fixed-point backward push of include/fora_hip.h
(twin_bwd_push), reverse_local_update_linear in f64 FIFO order as the reference writes it (fifo_bwd_push,
algo.h:703-751) and the BiPPR estimate (twin_bippr, bippr_query query.h:71-124); what the GPU tests need to know about
a push beyond its result (support_of, targets_over_cap, slot_of), the graph that puts a residue on the pop threshold and
the top-k order of a dense row (topk_of).  Everything fixed-point stays in Python ints, where a u64 wrap cannot hide."""
import math
from collections import deque

import numpy as np

BWD_ONE = 1 << 60
FIX_ONE = 1 << 62
U64 = (1 << 64) - 1


def bippr_setting(n, m, epsilon, rmax_scale=1.0):
    """(rmax, omega, W) in the reference's operand order, delta = pfail = 1/n."""
    delta = pfail = 1.0 / n
    rmax = epsilon * math.sqrt(m * 1.0 * delta / 3.0 / math.log(2.0 / pfail))
    rmax *= rmax_scale
    omega = rmax * 3 * math.log(2.0 / pfail) / delta / epsilon / epsilon
    return rmax, omega, math.ceil(omega)


_REV = {}


def reverse_csr(g):
    """In-edges of every node (graph.h's gr): rin[rin_ptr[v]:rin_ptr[v+1]] are the u with u -> v, duplicates kept."""
    key = id(g)
    if key not in _REV:
        src = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(g.row_ptr))
        dst = g.col[:src.size].astype(np.int64)
        order = np.argsort(dst, kind="stable")
        rin = src[order]
        rin_ptr = np.zeros(g.n + 1, dtype=np.int64)
        np.cumsum(np.bincount(dst, minlength=g.n), out=rin_ptr[1:])
        _REV[key] = (g, rin_ptr, rin)
    return _REV[key][1], _REV[key][2]


_PAIRS = {}


def _in_pairs(g):
    """In-edges as Python lists (the twin's inner loop reads nothing else): pairs[v] = [(u, outdeg(u)) for u -> v]."""
    key = id(g)
    if key not in _PAIRS:
        rin_ptr, rin = reverse_csr(g)
        ptr, rin, deg = rin_ptr.tolist(), rin.tolist(), np.diff(g.row_ptr).tolist()
        _PAIRS[key] = (g, [[(u, deg[u]) for u in rin[ptr[v]:ptr[v + 1]]] for v in range(g.n)])
    return _PAIRS[key][1]


def twin_bwd_push_sparse(g, t, rmax, alpha=0.2):
    """The level-synchronous push at 2^60 in Python ints: (reserve dict, residue dict, pops, relax, levels).  A level
    pops every node over thr; only a node that the level before added to can have risen over it, so those are the ones
    looked at.  The residue dict has a key for the target and for every node that ever got a non-zero increment."""
    pairs = _in_pairs(g)
    thr = math.floor(math.ldexp(rmax, 60))
    afix = int(math.ldexp(alpha, 62))
    t = int(t)
    r = [0] * g.n
    r[t] = BWD_ONE
    p = {}
    support = {t}
    pops = relax = levels = 0
    front = [t] if BWD_ONE > thr else []
    while front:
        levels += 1
        pops += len(front)
        pushes = []
        for v in front:
            x = r[v]
            keep = (x * afix) >> 62
            r[v] = 0
            p[v] = p.get(v, 0) + keep
            pushes.append((pairs[v], x - keep))
        touched = set()
        add = touched.add
        for pr, y in pushes:
            relax += len(pr)
            for u, d in pr:
                inc = y // d
                if inc:
                    r[u] += inc
                    add(u)
        support |= touched
        front = [u for u in touched if r[u] > thr]
    r = {v: r[v] for v in support}
    assert all(x <= thr for x in r.values())
    assert all(x <= U64 for x in r.values()) and all(x <= U64 for x in p.values())
    return p, r, pops, relax, levels


def twin_bwd_push_scan(g, t, rmax, alpha=0.2):
    """The same push written the plain way, as a cross-check of twin_bwd_push_sparse: every level scans every residue
    for the nodes over thr, on dicts, reading the reverse CSR directly.  Slower by the size of the support per level."""
    rin_ptr, rin = reverse_csr(g)
    deg = np.diff(g.row_ptr)
    thr = math.floor(math.ldexp(rmax, 60))
    afix = int(math.ldexp(alpha, 62))
    r = {int(t): BWD_ONE}
    p = {}
    pops = relax = levels = 0
    while True:
        front = [(v, x) for v, x in r.items() if x > thr]
        if not front:
            break
        levels += 1
        pops += len(front)
        pushes = []
        for v, x in front:
            keep = (x * afix) >> 62
            r[v] = 0
            p[v] = p.get(v, 0) + keep
            pushes.append((v, x - keep))
        for v, y in pushes:
            b, e = int(rin_ptr[v]), int(rin_ptr[v + 1])
            relax += e - b
            for u in rin[b:e].tolist():
                inc = y // int(deg[u])
                if inc:
                    r[u] = r.get(u, 0) + inc
    return p, r, pops, relax, levels


def support_of(r):
    """The nodes a push touched: the keys of the twin's residue dict (the target, and every node that got a non-zero
    increment).  Its size is what the LDS tier's table has to hold."""
    return set(r)


def targets_over_cap(supports, cap):
    """How many of the pushes (support sizes, one per target of a call, duplicates counted) outgrow an LDS table of
    `cap` entries.  cap 0 sends every target to the global tier, and every support holds its target."""
    return sum(1 for s in supports if s > cap)


def twin_bwd_push(g, t, rmax, alpha=0.2):
    """Dense u64 reserve and residue at 2^60 plus pops, relax and levels."""
    p, r, pops, relax, levels = twin_bwd_push_sparse(g, t, rmax, alpha)
    rsv = np.zeros(g.n, dtype=np.uint64)
    res = np.zeros(g.n, dtype=np.uint64)
    for v, x in p.items():
        rsv[v] = x
    for v, x in r.items():
        res[v] = x
    return dict(reserve=rsv, residue=res, pops=pops, relax=relax, levels=levels)


def entries_of(p, r):
    return sum(1 for x in p.values() if x) + sum(1 for x in r.values() if x)


def fifo_bwd_push(g, t, rmax, alpha=0.2):
    """reverse_local_update_linear (algo.h:703-751) in f64: FIFO queue, the target queued without a test, `break` on
    a popped residue < myeps, neighbours queued once their residue exceeds myeps.  Returns dense f64 reserve, residue."""
    rin_ptr, rin = reverse_csr(g)
    deg = np.diff(g.row_ptr)
    reserve = np.zeros(g.n)
    residue = np.zeros(g.n)
    inq = np.zeros(g.n, dtype=bool)
    q = deque([t])
    residue[t] = 1.0
    inq[t] = True
    while q:
        v = q.popleft()
        inq[v] = False
        if residue[v] < rmax:
            break
        reserve[v] += residue[v] * alpha
        rest = (1 - alpha) * residue[v]
        residue[v] = 0
        for u in rin[rin_ptr[v]:rin_ptr[v + 1]].tolist():
            residue[u] += rest / deg[u]
            if residue[u] > rmax and not inq[u]:
                inq[u] = True
                q.append(u)
    return reserve, residue


def bwd_all(g, rmax, alpha=0.2):
    """Sparse twin pushes of every target (shared by the sources of twin_bippr)."""
    return [twin_bwd_push_sparse(g, t, rmax, alpha)[:2] for t in range(g.n)]


def mc_slab(n, ends):
    """Walk slab at 2^-62 of walks j = 0 .. W-1 ending at ends[j]: floor(2^62 / W) + (j < 2^62 mod W) units each."""
    W = len(ends)
    base, rem = FIX_ONE // W, FIX_ONE % W
    return (np.bincount(ends, minlength=n).astype(np.uint64) * np.uint64(base)
            + np.bincount(ends[:rem], minlength=n).astype(np.uint64))


def twin_bippr(g, s, rmax, W, ends, alpha=0.2, pushes=None):
    """ppr[i] = p_i[s] + sum_v floor(c[v] * r_i[v] / 2^62) at 2^60 (u64 array), c the walk slab of the W endpoints."""
    assert len(ends) == W
    c = [int(x) for x in mc_slab(g.n, np.asarray(ends, dtype=np.int64))]
    if pushes is None:
        pushes = bwd_all(g, rmax, alpha)
    out = np.zeros(g.n, dtype=np.uint64)
    for i, (p, r) in enumerate(pushes):
        acc = p.get(int(s), 0)
        for v, x in r.items():
            if x and c[v]:
                acc += (c[v] * x) >> 62
        assert acc <= U64
        out[i] = acc
    return out


def threshold_graph():
    """(n, src, dst, target, neighbour) of the graph that puts a residue exactly on the pop threshold at alpha = 0.5:
    the target's single in-neighbour has out-degree 2, so the target's pop keeps floor(2^60 * 2^61 / 2^62) = 2^59 and
    the neighbour receives floor(2^59 / 2) = 2^58 = 0.25 * 2^60 exactly.  The neighbour has an in-neighbour of its own,
    so whether it popped shows in every counter."""
    #   3 -> 1,  1 -> 0 (the target),  1 -> 2
    return 4, np.array([1, 1, 3], dtype=np.int32), np.array([0, 2, 1], dtype=np.int32), 0, 1


def slot_of(u, bits=11):
    """Home slot of node u in the LDS tier's table (fora_bwd.h: (u * 0x9E3779B1) >> (32 - BWD_TAB_BITS), 32-bit)."""
    return ((np.asarray(u, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)


def topk_of(fix, k, frac=60):
    """(ids, scores) of a dense fixed-point row: score descending, ties id ascending, padded with (0, 0.0)."""
    nz = np.flatnonzero(fix)
    order = sorted(nz.tolist(), key=lambda v: (-int(fix[v]), v))[:k]
    ids = np.zeros(k, dtype=np.int32)
    sc = np.zeros(k, dtype=np.float64)
    ids[:len(order)] = order
    sc[:len(order)] = [math.ldexp(int(fix[v]), -frac) for v in order]
    return ids, sc
