"""The SWEEP CUT contract of include/fora_hip.h in plain Python ints, with nothing from the library: a sort, a dict of ranks,
a difference array and an exact fraction compare.  sweep_brute recomputes every prefix from set membership instead."""
import math
import struct

import numpy as np

FIX_ONE = 1 << 62


def thr_fix_of(t):
    return 1 if t <= 0 else max(1, math.ceil(math.ldexp(t, 62)))


def _order(row, deg, thr):
    support = [int(v) for v in np.flatnonzero(np.asarray(row) >= np.uint64(thr))]
    key = {v: int(row[v]) // max(int(deg[v]), 1) for v in support}
    return sorted(support, key=lambda v: (-key[v], v)), key


def _best(cut, vol, nnz):
    """(best, cut, vol, den, conductance): the prefix of least cut / den over den > 0, exact, ties to the smaller prefix"""
    b = None
    for j in range(len(cut)):
        den = min(vol[j], nnz - vol[j])
        if den > 0 and (b is None or cut[j] * b[3] < b[1] * den):
            b = (j + 1, cut[j], vol[j], den)
    if b is None:
        return 0, 0, 0, 0, 1.0
    return b + (float(b[1]) / float(b[3]),)


def sweep_row(row, row_ptr, col, thr, max_size=0):
    """row: the n fixed-point words of one ppr row.  Returns a dict: len, order, cut, vol (lists of L ints), best, cut_best,
    vol_best, den, conductance."""
    deg = np.diff(row_ptr)
    nnz = int(row_ptr[-1])
    order, _ = _order(row, deg, thr)
    n_sup = len(order)
    L = n_sup if max_size <= 0 else min(n_sup, int(max_size))
    order = order[:L]
    rank = {v: i for i, v in enumerate(order)}
    diff = [0] * L
    for i, u in enumerate(order):
        for v in col[int(row_ptr[u]):int(row_ptr[u + 1])]:
            r = rank.get(int(v), -1)
            if r < 0 or r > i:
                diff[i] += 1
                if r > i:
                    diff[r] -= 1
    cut, vol, c, s = [], [], 0, 0
    for i, u in enumerate(order):
        c += diff[i]
        s += int(deg[u])
        cut.append(c)
        vol.append(s)
    best, cb, vb, den, cond = _best(cut, vol, nnz)
    return {"len": n_sup, "order": order, "cut": cut, "vol": vol, "best": best, "cut_best": cb, "vol_best": vb, "den": den,
            "conductance": cond}


def dangling_row(s):
    """the row of a dangling source: the single entry (s, 2^62), no prefix with a denominator"""
    return {"len": 1, "order": [int(s)], "cut": [0], "vol": [0], "best": 0, "cut_best": 0, "vol_best": 0, "den": 0, "conductance": 1.0}


def sweep_brute(row, row_ptr, col, thr, max_size=0):
    """the same profile with cut and vol of every prefix recomputed from set membership"""
    deg = np.diff(row_ptr)
    nnz = int(row_ptr[-1])
    order, _ = _order(row, deg, thr)
    n_sup = len(order)
    L = n_sup if max_size <= 0 else min(n_sup, int(max_size))
    order = order[:L]
    cut, vol = [], []
    for j in range(L):
        S = set(order[:j + 1])
        cut.append(sum(1 for u in S for v in col[int(row_ptr[u]):int(row_ptr[u + 1])] if int(v) not in S))
        vol.append(sum(int(deg[u]) for u in S))
    best, cb, vb, den, cond = _best(cut, vol, nnz)
    return {"len": n_sup, "order": order, "cut": cut, "vol": vol, "best": best, "cut_best": cb, "vol_best": vb, "den": den,
            "conductance": cond}


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def minimisers(cut, vol, nnz):
    """0-based positions of the prefixes that attain the least cut / den over den > 0, exactly (cross-multiplied ints)"""
    best, out = None, []
    for j in range(len(cut)):
        den = min(vol[j], nnz - vol[j])
        if den <= 0:
            continue
        if best is None or cut[j] * best[1] < best[0] * den:
            best, out = (cut[j], den), [j]
        elif cut[j] * best[1] == best[0] * den:
            out.append(j)
    return out


def keys_in_order(row, row_ptr, order):
    deg = np.diff(row_ptr)
    return [int(row[v]) // max(int(deg[v]), 1) for v in order]


def tied_boundaries(keys, step):
    """(boundaries b = step, 2 * step, ... < len(keys) with keys[b - 1] == keys[b], all such boundaries)"""
    bs = range(step, len(keys), step)
    return sum(1 for b in bs if keys[b - 1] == keys[b]), len(bs)


# ---- rows and graphs that real PPR rows never give (equal keys, equal conductances, crowded degree classes)
TIE_SEEDS = (8801, 8802, 8803)   # tie_heavy_row over the `small` preset with dangling nodes: see tests/test_sweep_cpu.py
HUB_CLASSES = (121, 135)         # hubs_first_row there: nodes of outdeg >= 256 and of 64 .. 255 among the first 256


def random_row(rng, n, row_ptr, density=0.6):
    """a sparse row with equal keys on several ids: words of the form q * max(deg, 1) (+ a remainder below deg)"""
    deg = np.maximum(np.diff(row_ptr), 1)
    row = np.zeros(n, dtype=np.uint64)
    on = rng.random(n) < density
    q = rng.integers(1, 6, size=n).astype(np.uint64) << np.uint64(40)   # few distinct quotients: ties by id
    rem = rng.integers(0, 1 << 20, size=n).astype(np.uint64) % deg.astype(np.uint64)
    row[on] = (q * deg.astype(np.uint64) + rem)[on]
    return row


def row_of_length(row, length):
    """`row` with only its `length` first non-zero words (by id) kept"""
    out = np.zeros_like(row)
    keep = np.flatnonzero(row)[:length]
    assert keep.size == length
    out[keep] = row[keep]
    return out


def tie_heavy_row(n, row_ptr, seed):
    """random_row at density 0.8: on a graph of 32 000 nodes about 25 600 entries under 5 distinct keys"""
    return random_row(np.random.Generator(np.random.PCG64(seed)), n, row_ptr, density=0.8)


def edge_words_row(n, row_ptr, seed, count=1200):
    """Four groups of `count` nodes each (fewer where the graph has fewer) and one more node:
      keys c + (k << 33), k = 1 .. 7: they differ only above bit 32       keys (9 << 33) + k, k < 2^20: only below it
      keys 0 on real entries: a word in [1, outdeg) on a node of outdeg >= 2      keys 1 on dangling nodes (word 1)
      the word 2^62 on a node of outdeg 1 (the largest key a row can hold).
    Returns (row, ids of the key-0 entries ascending)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    deg = np.diff(row_ptr).astype(np.uint64)
    row = np.zeros(n, dtype=np.uint64)
    one = np.flatnonzero(deg == 1)
    live = rng.permutation(np.flatnonzero(deg >= 2))
    hi, lo, zero = live[:count], live[count:2 * count], np.sort(live[2 * count:3 * count])
    assert one.size and zero.size >= 8
    row[hi] = ((rng.integers(1, 8, size=hi.size).astype(np.uint64) << np.uint64(33)) + np.uint64(12345)) * deg[hi]
    row[lo] = ((np.uint64(9) << np.uint64(33)) + rng.integers(0, 1 << 20, size=lo.size).astype(np.uint64)) * deg[lo]
    row[zero] = 1 + rng.integers(0, 1 << 30, size=zero.size).astype(np.uint64) % (deg[zero] - np.uint64(1))
    row[np.flatnonzero(deg == 0)[:count]] = 1
    row[one[0]] = FIX_ONE
    assert (row[zero] < deg[zero]).all() and (row[zero] > 0).all()
    return row, zero.astype(np.int32)


def hubs_first_row(row_ptr):
    """full support, key(v) = (outdeg(v) + 1) << 20: the order is the nodes by descending degree, ties by id"""
    deg = np.diff(row_ptr).astype(np.uint64)
    return ((deg + np.uint64(1)) << np.uint64(20)) * np.maximum(deg, np.uint64(1))


def _csr(n, src, dst):
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    o = np.lexsort((dst, src))
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=row_ptr[1:])
    return row_ptr, dst[o].astype(np.int32)


def descending_row(n):
    """the keys (n - v) << 20, the row itself on a graph whose degrees are all 1 (the caller multiplies by another common
    degree): the order is 0 .. n - 1"""
    return (np.uint64(n) - np.arange(n, dtype=np.uint64)) << np.uint64(20)


def ring_graph(m):
    """the bidirectional ring on m nodes (all degrees 2) and the row whose order is 0 .. m - 1.  Every proper prefix has cut
    2 and vol 2 (j + 1): for odd m the prefixes of (m - 1) / 2 and (m + 1) / 2 nodes share the largest denominator m - 1.
    Returns (n, row_ptr, col, row)."""
    u = np.arange(m, dtype=np.int64)
    row_ptr, col = _csr(m, np.concatenate([u, u]), np.concatenate([(u + 1) % m, (u - 1) % m]))
    return m, row_ptr, col, descending_row(m) * np.uint64(2)


def pair_graph(k):
    """k disjoint 2-cycles {2 i, 2 i + 1} and the row whose order is 0 .. 2 k - 1: every prefix of even size has cut 0.
    Returns (n, row_ptr, col, row)."""
    u = np.arange(2 * k, dtype=np.int64)
    row_ptr, col = _csr(2 * k, u, u ^ 1)
    return 2 * k, row_ptr, col, descending_row(2 * k)


def chord_ring_graph(n=40000, chords=2000, hub_deg=300, seed=20261020):
    """A bidirectional ring on n nodes, `chords` random chords (both directions), and node 0 with `hub_deg` further
    out-edges (one way): a graph whose full-support row is longer than 32 768.  Returns (n, row_ptr, col)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    u = np.arange(n, dtype=np.int64)
    a, b = rng.integers(0, n, size=chords), rng.integers(0, n, size=chords)
    hub = rng.choice(np.arange(2, n - 1), size=hub_deg, replace=False)
    src = np.concatenate([u, u, a, b, np.zeros(hub_deg, dtype=np.int64)])
    dst = np.concatenate([(u + 1) % n, (u - 1) % n, b, a, hub])
    keep = src != dst
    e = np.unique(src[keep] * n + dst[keep])
    row_ptr, col = _csr(n, e // n, e % n)
    return n, row_ptr, col


# ---- inputs of k_sweep_scan alone: a difference array and a per-position volume array of one row
def scan_ref(diff, vol, nnz):
    """both prefix sums and the best prefix in Python ints: cut, vol (lists), best, cut_best, vol_best, den, edges"""
    cut, vs, c, s = [], [], 0, 0
    for d, v in zip(diff, vol):
        c += int(d)
        s += int(v)
        assert c >= 0
        cut.append(c)
        vs.append(s)
    assert s <= nnz
    best, cb, vb, den, _ = _best(cut, vs, nnz)
    return {"cut": cut, "vol": vs, "best": best, "cut_best": cb, "vol_best": vb, "den": den, "edges": s}


SCAN_LENGTHS = (1, 4, 5, 1024, 1025, 5000)
# (p, q) of a planted pair: inside one lane's four positions, in two waves, either side of a 1024-position step (k_sweep_scan)
SCAN_PLACES = {"lane": (4, 6), "lane0": (1, 2), "waves": (100, 700), "step": (1023, 1024), "steps": (500, 4500)}
SCAN_KINDS = ("tie", "low_p", "low_q", "high_p", "high_q")
_M64 = (1 << 64) - 1


def _from_prefixes(cut, vol):
    diff = np.array([cut[0]] + [cut[j] - cut[j - 1] for j in range(1, len(cut))], dtype=np.int64)
    v = np.array([vol[0]] + [vol[j] - vol[j - 1] for j in range(1, len(vol))], dtype=np.uint64)
    return diff, v


def scan_background(rng, L, unit=None):
    """cuts in [2^44, 2^45], volumes of 2^39 .. 2^40 per position (multiples of `unit` when given): every prefix has
    cut / vol >= 2^44 / (L * 2^40), above 2^-9 for L <= 5000"""
    cut = [int(x) for x in rng.integers(1 << 44, (1 << 45) + 1, size=L)]
    if unit is None:
        step = [int(x) for x in rng.integers(1 << 39, (1 << 40) + 1, size=L)]
    else:
        step = [unit * int(x) for x in rng.integers(1, 3, size=L)]
        assert max(step) <= 1 << 40
    vol = list(np.cumsum(np.array(step, dtype=object)))
    return cut, vol


def scan_planted(rng, L, kind, p, q):
    """A row whose two best prefixes are p and q (0-based, p < q < L), far below the background (cut / vol <= 2^-10), under
    nnz = 2^62 (den = vol everywhere).  Returns (diff, vol, nnz, winner):
      tie     cut_p / vol_p == cut_q / vol_q exactly (both are h x, g x and h y, g y): the 128-bit products are equal, p wins
      low_*   the products differ in the high word and their low words order the other way round; * wins
      high_*  the products agree in the high word and differ in the low word; * wins"""
    assert 0 <= p < q < L
    nnz = 1 << 62
    for _ in range(10000):
        if kind == "tie":
            g = (int(rng.integers(1 << 38, 1 << 39)) | 1)
            cut, vol = scan_background(rng, L, unit=g)
            h = int(rng.integers(1 << 24, 1 << 25))
            cut[p], cut[q] = h * (vol[p] // g), h * (vol[q] // g)
            winner = p
        else:
            cut, vol = scan_background(rng, L)
            da, db = vol[p], vol[q]
            ca = int(rng.integers(1 << 26, 1 << 28))
            left = ca * db
            if kind.startswith("high"):
                cb = left // da + (1 if kind == "high_p" else 0)
            else:
                cb = left // da + int(rng.integers(1, 1 << 24)) * (1 if kind == "low_p" else -1)
            right = cb * da
            if not (0 < cb <= 1 << 45) or left == right:
                continue
            if kind.startswith("high") and left >> 64 != right >> 64:
                continue
            if kind.startswith("low") and (left >> 64 == right >> 64 or ((left & _M64) < (right & _M64)) == (left < right)):
                continue
            cut[p], cut[q] = ca, cb
            winner = p if left < right else q
            assert winner == (p if kind.endswith("_p") else q)
        assert cut[p] * vol[q] >> 64 > 0 and max(cut) <= 1 << 45 and cut[p] << 10 <= vol[p] and cut[q] << 10 <= vol[q]
        diff, v = _from_prefixes(cut, vol)
        assert int(v.max()) <= 1 << 40 and int(diff.min()) < -(1 << 40)
        return diff, v, nnz, winner
    raise AssertionError("no such pair found")


def scan_plain(rng, L, nnz_slack=0):
    """the background alone under nnz = the row's volume + nnz_slack: denominators from both sides, 0 at the end without slack"""
    cut, vol = scan_background(rng, L)
    diff, v = _from_prefixes(cut, vol)
    return diff, v, vol[-1] + nnz_slack


def planted_graph(seed=20261019, small=300, big=1699, nbrs=4, cross=60):
    """A symmetric two-block graph: every node draws `nbrs` random partners inside its block (about 2 * nbrs neighbours per
    node once the edges are mirrored), `cross` edges join the blocks, ids are permuted.  Returns (n, row_ptr, col, members of
    the small block)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = small + big
    pairs = set()
    for lo, size in ((0, small), (small, big)):
        for u in range(lo, lo + size):
            for v in lo + rng.choice(size, size=nbrs, replace=False):
                if int(v) != u:
                    pairs.add((min(u, int(v)), max(u, int(v))))
    while cross > 0:
        u, v = int(rng.integers(0, small)), int(small + rng.integers(0, big))
        if (u, v) not in pairs:
            pairs.add((u, v))
            cross -= 1
    perm = rng.permutation(n)
    e = np.array(sorted(pairs), dtype=np.int64)
    src = np.concatenate([perm[e[:, 0]], perm[e[:, 1]]])
    dst = np.concatenate([perm[e[:, 1]], perm[e[:, 0]]])
    o = np.lexsort((dst, src))
    src, dst = src[o], dst[o]
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=row_ptr[1:])
    return n, row_ptr, dst.astype(np.int32), np.sort(perm[:small]).astype(np.int32)
