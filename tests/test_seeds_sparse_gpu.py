"""Sparse rows of seed sets on the GPU (fora_hip_seeds_sparse_batch, Engine.query_seeds_sparse): the set rows thresholded
after the sum and compacted on the device.  The expected rows never pass through the new code: they are the Engine.query_fix
rows of the individual seeds (pinned to oracle/fora_twin.c by test_hip_parity_gpu.py), folded by tests/seeds_ref.py and
thresholded in Python ints.  Every comparison is an equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import seeds_outputs_ref as so
import seeds_ref as sr
from fora_amd import ForaError, synth

pytestmark = pytest.mark.gpu
THRESHOLDS = (None, 0.0, 1e-3, 1.0)   # None: 1 / n; 0: every non-zero word


@pytest.fixture(scope="module")
def odd(oracle):
    """n odd: every other row of the accumulator block starts at an odd word (no 16-byte alignment)."""
    src, dst = synth.rmat_graph(1999, 16000, 20260118)
    return oracle.Graph.from_edges(1999, 16000, src, dst)


def check(g, sets, expect, t, out, dedup=1):
    """one call's dict against the expected set rows"""
    thr = so.thr_fix_of(1.0 / g.n if t is None else t)
    row_ptr, ids, fix = so.csr_of(expect, thr)
    assert out["row_ptr"].dtype == np.int64 and out["ids"].dtype == np.int32 and out["fix"].dtype == np.uint64
    assert out["row_ptr"].tolist() == row_ptr
    assert out["ids"].tolist() == ids
    assert out["fix"].tolist() == fix
    assert out["vals"].dtype == np.float64 and np.array_equal(out["vals"], np.ldexp(out["fix"].astype(np.float64), -62))
    assert out["row_sum_fix"].tolist() == [sum(r) for r in expect]   # over the whole row, not over the kept part
    for name, want in so.counts(g, sets, dedup).items():
        assert out["stats"][name] == want, name
    assert out["stats"]["batches"] >= (1 if out["stats"]["queries"] else 0) and out["stats"]["combine_ms"] >= 0
    sp = out["sparse"]
    assert sp["entries"] == len(ids) and sp["max_row"] == max(np.diff(row_ptr)) and sp["thr_fix"] == thr
    assert sp["batches"] >= 1 and sp["compact_ms"] >= 0


def both(engine, g, c, t=None, dedup=1, with_idx=False):
    for k, w in (("u", None), ("w", c.weights)):
        out = engine.query_seeds_sparse(c.sets, weights=w, with_idx=with_idx, threshold=t, want_fix=True)
        check(g, c.sets, c.expect[k], t, out, dedup)
    return out


@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling", "odd"])
def test_csr_equals_the_thresholded_set_rows(engine, request, gname):
    g = request.getfixturevalue(gname)
    so.load(engine, g)
    c = so.reference(engine, g)
    for t in THRESHOLDS:
        out = both(engine, g, c, t)
    assert out["ids"].size == 0 or t != 1.0 or all(x == so.ONE for x in out["fix"].tolist())   # threshold 1.0: whole words only
    zero = engine.query_seeds_sparse(c.sets, threshold=0.0, want_fix=True)
    assert zero["fix"].tolist() == [x for r in c.expect["u"] for x in r if x]   # every non-zero word
    assert np.array_equal(zero["ids"][zero["row_ptr"][1]:zero["row_ptr"][2]], zero["ids"][zero["row_ptr"][-3]:zero["row_ptr"][-2]])  # duplicate sets
    flat = (np.cumsum([0] + [len(s) for s in c.sets]), np.concatenate(c.sets))  # the (set_ptr, seeds) form, flat weights
    again = engine.query_seeds_sparse(flat, weights=np.concatenate(c.weights), want_fix=True)
    check(g, c.sets, c.expect["w"], None, again)
    nofix = engine.query_seeds_sparse(c.sets)
    assert nofix["fix"] is None and nofix["ids"].size == nofix["vals"].size == int(nofix["row_ptr"][-1])


CONFIGS = {
    "batch4": dict(batch=4), "batch1": dict(batch=1), "dedup0": dict(dedup=0), "wide": dict(force_wide=1),
    "rows1": dict(seeds_rows=1), "rows3": dict(seeds_rows=3), "rows256": dict(seeds_rows=256),
    "rows3_batch4_dedup0_wide": dict(seeds_rows=3, batch=4, dedup=0, force_wide=1),
}


@pytest.mark.parametrize("gname", ["tiny", "tiny_dangling", "odd"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_same_bits_whatever_the_batching_dedup_layout_and_chunk(engine, request, gname, config):
    """seeds_rows 1 and 3 on the graph of 1999 nodes are the alignment rule's case: a chunk of an odd number of rows would
    start the next one at an odd word of the block."""
    g = request.getfixturevalue(gname)
    so.load(engine, g)
    c = so.reference(engine, g)
    kw = dict(CONFIGS[config])
    batch, dedup = kw.pop("batch", 0), kw.pop("dedup", 1)
    try:
        engine.set_option("seeds_dedup", dedup)
        for name, v in kw.items():
            engine.set_option(name, v)
        engine.set_batch(batch)
        out = both(engine, g, c, None, dedup)
        both(engine, g, c, 0.0, dedup)
        if batch == 4:
            assert out["stats"]["batches"] == -(-out["stats"]["queries"] // 4) >= 3
        rows = kw.get("seeds_rows", 256)
        rows += rows & g.n & 1   # an odd n: rounded up to even
        assert out["sparse"]["batches"] == -(-len(c.sets) // rows)
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


def test_a_singleton_equals_query_sparse(engine, tiny_dangling):
    g = tiny_dangling
    so.load(engine, g)
    live, dang = so.pick(g, 3, 621), so.pick(g, 2, 622, want_dangling=True)
    srcs = live[:2] + dang[:1] + live[2:] + dang[1:]
    assert len(dang) == 2
    for t in (None, 0.0):
        row_ptr, ids, vals, fix, _, sp = engine.query_sparse(np.array(srcs, dtype=np.int32), threshold=t, want_fix=True)
        out = engine.query_seeds_sparse([[s] for s in srcs], threshold=t, want_fix=True)
        assert np.array_equal(out["row_ptr"], row_ptr) and np.array_equal(out["ids"], ids)
        assert np.array_equal(out["fix"], fix) and np.array_equal(out["vals"], vals)
        assert out["sparse"]["entries"] == sp["entries"] and out["sparse"]["max_row"] == sp["max_row"]
        for i, s in enumerate(srcs):
            if g.deg[s] == 0:   # a dangling seed: the one entry (s, 2^62)
                lo, hi = int(out["row_ptr"][i]), int(out["row_ptr"][i + 1])
                assert hi - lo == 1 and int(out["ids"][lo]) == s and int(out["fix"][lo]) == so.ONE
        assert out["row_sum_fix"].tolist() == [so.ONE] * len(srcs)


def test_the_sum_keeps_a_node_that_every_thresholded_seed_row_has_lost(engine, tiny):
    """The (v, thr) of test_seeds_outputs_cpu.py on the GPU's own rows, at exactly that threshold."""
    g = tiny
    so.load(engine, g)
    seeds = so.pick(g, 3, 611)
    fix, _, _ = engine.query_fix(np.array(seeds, dtype=np.int32), want_residue=False)
    rows = [r.tolist() for r in fix]
    wfix = sr.uniform_wfix(3)
    row = sr.combine(rows, wfix)
    found = so.lifted_node(rows, wfix)
    assert found is not None
    v, thr, terms = found
    assert all(t < thr for t in terms) and thr == row[v] and v not in so.merge_thresholded(rows, wfix, thr)
    t = float(thr) * 2.0 ** -62
    assert so.thr_fix_of(t) == thr
    out = engine.query_seeds_sparse([seeds], threshold=t, want_fix=True)
    check(g, [seeds], [row], t, out)
    ids = out["ids"].tolist()
    assert v in ids and int(out["fix"][ids.index(v)]) == row[v]
    up = engine.query_seeds_sparse([seeds], threshold=float(thr + 1) * 2.0 ** -62, want_fix=True)   # one unit more: v is gone
    assert up["sparse"]["thr_fix"] == thr + 1 and v not in up["ids"].tolist()


def _raw_fetch(engine, ids, vals, fix, cap):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return engine._lib.fora_hip_sparse_fetch(engine._ctx, p(ids), p(vals), p(fix), C.c_uint64(cap))


def test_lifetime_of_the_held_result(engine, tiny_dangling):
    g = tiny_dangling
    so.load(engine, g)
    c = so.reference(engine, g)
    srcs = np.array(c.sets[-1][:4], dtype=np.int32)
    held_sweep = engine.sweep(srcs, want_profile=True)
    first = engine.query_sparse(srcs, want_fix=True)
    out = engine.query_seeds_sparse(c.sets, want_fix=True)   # replaces the held sparse result
    check(g, c.sets, c.expect["u"], None, out)
    e = int(out["row_ptr"][-1])
    assert e != first[-1]["entries"]
    ids, vals, fix = np.zeros(e, np.int32), np.zeros(e, np.float64), np.zeros(e, np.uint64)
    assert _raw_fetch(engine, ids, vals, fix, e) == 0
    assert np.array_equal(ids, out["ids"]) and np.array_equal(vals, out["vals"]) and np.array_equal(fix, out["fix"])
    # the sweep result held before the call is untouched by it
    n_e = int(held_sweep["row_ptr"][-1])
    sids, scut, svol = engine.sweep_fetch(n_e)
    assert np.array_equal(sids, held_sweep["ids"]) and np.array_equal(scut, held_sweep["cut"]) and np.array_equal(svol, held_sweep["vol"])
    # the sparse result survives other calls, the dense seed-set call among them
    engine.query(srcs, want_ppr=False)
    engine.query_seeds(c.sets, want_fix=False)
    f2 = np.zeros(e + 3, np.uint64)
    assert _raw_fetch(engine, None, None, f2, e + 3) == 0 and np.array_equal(f2[:e], out["fix"]) and (f2[e:] == 0).all()
    # a small cap: refused, nothing written
    i3, f3 = np.full(e, -7, np.int32), np.full(e, 77, np.uint64)
    assert _raw_fetch(engine, i3, None, f3, e - 1) == -1 and (i3 == -7).all() and (f3 == 77).all()
    engine.sparse_clear()
    assert _raw_fetch(engine, i3, None, f3, 1 << 40) == -1 and (i3 == -7).all()
    sids, _, _ = engine.sweep_fetch(n_e)   # ... and the clear leaves the sweep result alone too
    assert np.array_equal(sids, held_sweep["ids"])
    engine.sweep_clear()


def _raw(engine, set_ptr, seeds, weights, ns, with_idx=0, thr=0.0, row_ptr=None, sums=None):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return engine._lib.fora_hip_seeds_sparse_batch(engine._ctx, p(set_ptr), p(seeds), p(weights), C.c_int(ns), C.c_int(with_idx),
                                                   C.c_double(thr), p(row_ptr), p(sums), None, None)


def test_argument_errors_leave_the_engine_as_it_was(engine, tiny):
    g = tiny
    so.load(engine, g)
    a, b = so.pick(g, 2, 604)
    probe = np.array([a, b], dtype=np.int32)
    base, _ = engine.query(probe)
    good = engine.query_seeds_sparse([[a, b]], want_fix=True)
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
        "nan weight": (i64(0, 2), i32(a, b), f64(1.0, float("nan")), 1, 0, 0.0, rp),
        "zero sum": (i64(0, 1, 3), i32(a, a, b), f64(1.0, 0.0, 0.0), 2, 0, 0.0, rp),
        "with_idx without an index": (i64(0, 1), i32(a), None, 1, 1, 0.0, rp),
    }
    for name, (set_ptr, seeds, weights, ns, with_idx, thr, row_ptr) in cases.items():
        assert _raw(engine, set_ptr, seeds, weights, ns, with_idx, thr, row_ptr) == -1, name  # FORA_E_ARG
        assert (rp == -5).all(), name
        assert _raw_fetch(engine, None, None, None, 1 << 40) == -1, name   # every call, a failed one too, ends the held result
        again, _ = engine.query(probe)
        assert np.array_equal(again, base), name
    with pytest.raises(ForaError) as e:  # ... and through the binding
        engine.query_seeds_sparse([[a], []])
    assert e.value.code == -1
    with pytest.raises(ValueError):
        engine.query_seeds_sparse([[a, b]], weights=[[1.0]])
    later = engine.query_seeds_sparse([[a, b]], want_fix=True)   # a later correct call is what it was
    for name in ("row_ptr", "ids", "fix", "vals", "row_sum_fix"):
        assert np.array_equal(later[name], good[name]), name
    engine.sparse_clear()


def test_empty_call(engine, tiny):
    so.load(engine, tiny)
    engine.query_sparse(np.array(so.pick(tiny, 1, 605), dtype=np.int32))
    out = engine.query_seeds_sparse([], want_fix=True)
    assert out["row_ptr"].tolist() == [0] and out["ids"].size == out["vals"].size == out["fix"].size == out["row_sum_fix"].size == 0
    assert all(v == 0 for v in out["stats"].values()) and all(v == 0 for v in out["sparse"].values())
    assert _raw_fetch(engine, None, None, None, 0) == 0   # an empty result is held
    rp = np.full(1, -5, dtype=np.int64)
    assert _raw(engine, None, None, None, 0, row_ptr=rp) == 0 and rp[0] == 0   # nothing to read: null arrays are fine
    engine.sparse_clear()
    assert _raw_fetch(engine, None, None, None, 0) == -1


def test_device_fetch():
    """Engine.query_seeds_sparse(device=True) in a fresh child (tests/seeds_sparse_device_child.py): torch tensors and the
    library must live on one HIP runtime, so the child imports torch before the library is loaded."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "seeds_sparse_device_child.py")], capture_output=True, text=True,
                       timeout=300, cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "seeds sparse device ok" in r.stdout
