"""SUBGRAPH POOL on the GPU, through the C ABI (the contract of include/fora_hip_pool.h): the maximum / minimum over the groups of the
held subgraph with its arg, and the gradient, are the numpy twin's (tests/subgraph_pool_ref.py) bit for bit under every value of
"sub_short", "prop_segs" and "propt_lds_cap", by row and by column, for every element type -- every comparison here is an equality
of bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import narrow_ref
import propagate_ref as pr
import propagate_values_ref as pv
import subgraph_pool_ref as pool
import subgraph_prop_ref as sr
from test_subgraph_prop_gpu import CONFIGS, Crafted, _eq, _p

pytestmark = pytest.mark.gpu
E_ARG, NC, D, F = -1, sr.CRAFTED_NC, 64, 21   # (F: the first filler node -- entry k of every crafted group reads node F + k)


@pytest.fixture(scope="module")
def crafted():
    c = Crafted()
    yield c
    c.eng.close()


@pytest.fixture(scope="module")
def ref(crafted):
    """the operands and the twin's results at d = 64, made once (a narrower call is the first d columns): "ties" draws from six values,
    so nearly every group has ties and both zeros meet in either order; "nan" also has infinities at the entries 10 and 20 of every
    group and NaNs behind them -- at entry 40, at 64 (the last of the group of 65), at 256 (the last of 257) and at 260"""
    sub_ptr, sub_col = crafted.sub[0], crafted.sub[1]
    rng = np.random.Generator(np.random.PCG64(11300))
    ties = rng.choice(np.array([-2, -1, -0.0, 0.0, 1, 2], dtype=np.float32), size=(NC, D))
    nan = ties.copy()
    nan[F + 10], nan[F + 20], nan[F + 260] = np.inf, -np.inf, np.nan
    nan[F + 40, ::2], nan[F + 64, 1::2], nan[F + 256, ::3] = np.nan, np.nan, np.nan
    r = {"X": {"ties": ties, "nan": nan}, "G": pv.distinct_values(rng, NC * D, np.float32).reshape(NC, D)}
    r["fwd"] = {(x, op, by): pool.forward(sub_ptr, sub_col, X, op=op, by=by) for x, X in r["X"].items() for op in ("max", "min") for by in ("row", "col")}
    r["bwd"] = {by: pool.backward(sub_ptr, sub_col, r["G"], r["fwd"]["ties", "max", by][2], by=by) for by in ("row", "col")}
    return r


@pytest.mark.parametrize("d", [1, 3, 33, 64])
@pytest.mark.parametrize("by", ["row", "col"])
@pytest.mark.parametrize("op", ["max", "min"])
def test_forward_against_the_twin_under_every_option(crafted, ref, op, by, d):
    eng = crafted.eng
    try:
        for config in CONFIGS:
            crafted.take(config)
            for x, X in ref["X"].items():
                w64, w32, warg = ref["fwd"][x, op, by]
                o32, o64, arg, st = eng.subgraph_pool(np.ascontiguousarray(X[:, :d]), op=op, by=by, want32=True, want64=True)
                _eq(o64, np.ascontiguousarray(w64[:, :d]), f"out64 {config} {x}")
                _eq(o32, np.ascontiguousarray(w32[:, :d]), f"out32 {config} {x}")
                _eq(arg, np.ascontiguousarray(warg[:, :d]), f"arg {config} {x}")
                cap = 256 if config[0] is None else config[0]
                lens = np.diff(crafted.sub[0]) if by == "row" else np.bincount(crafted.sub[1], minlength=NC)
                assert st["long_rows"] == int((lens > cap).sum()) > 0 and st["chunks"] == 1 and st["x_on_device"] == 0, (config, st)
    finally:
        eng.reset_options()


@pytest.mark.parametrize("d", [3, 64])
@pytest.mark.parametrize("by", ["row", "col"])
def test_backward_against_the_twin_under_every_option(crafted, ref, by, d):
    eng = crafted.eng
    G, arg = np.ascontiguousarray(ref["G"][:, :d]), np.ascontiguousarray(ref["fwd"]["ties", "max", by][2][:, :d])
    w64, w32 = (np.ascontiguousarray(a[:, :d]) for a in ref["bwd"][by])
    assert w64.any()
    try:
        for config in CONFIGS:
            crafted.take(config)
            o32, o64, st = eng.subgraph_pool_bwd(G, arg, by=by, want32=True, want64=True)
            _eq(o64, w64, f"out64 {config}")
            _eq(o32, w32, f"out32 {config}")
            if config[1] is not None:
                assert st["long_rows"] and st["chunks"] > 1, (config, st)
    finally:
        eng.reset_options()


def test_backward_with_a_stale_arg_adds_nothing(crafted, ref):
    """every group is given the arg of the group before it: edges of other groups, and the -1 of the empty ones"""
    eng, (sub_ptr, sub_col) = crafted.eng, crafted.sub[:2]
    crafted.take((64, 2, None))
    try:
        for by in ("row", "col"):
            stale = np.roll(ref["fwd"]["ties", "max", by][2][:, :33], 1, axis=0)
            assert (stale >= 0).sum() > 700 and (stale == -1).any()
            o32, o64, _ = eng.subgraph_pool_bwd(np.ascontiguousarray(ref["G"][:, :33]), stale, by=by, want32=True, want64=True)
            _eq(o64, pool.backward(sub_ptr, sub_col, ref["G"][:, :33], stale, by=by)[0], f"stale {by}")
            assert not o64.any() and not o32.any() and not np.signbit(o64).any()
    finally:
        eng.reset_options()


@pytest.mark.parametrize("kind", ["bf16", narrow_ref.F16, narrow_ref.E4M3, narrow_ref.E5M2])
def test_narrow_operands_against_the_widened_f32_call(crafted, kind):
    eng, d = crafted.eng, 32
    rng = np.random.Generator(np.random.PCG64(11310))
    crafted.take((64, 2, None))
    try:
        if kind == "bf16":
            codes = pr.to_bf16_bits(pv.distinct_values(rng, NC * d, np.float32).reshape(NC, d))
            operand, keyword = codes, True
        else:
            codes = narrow_ref.moderate_codes(rng, kind, (NC, d))
            operand, keyword = narrow_ref.as_operand(kind, codes)
        wide = sr.widen32(codes, kind)
        for by in ("row", "col"):
            got = eng.subgraph_pool(operand, op="min", by=by, bf16=keyword, want32=True, want64=True)
            want = eng.subgraph_pool(wide, op="min", by=by, want32=True, want64=True)
            for a, b, name in zip(got[:3], want[:3], ("out32", "out64", "arg")):
                _eq(a, b, f"{kind} {by} {name}")
            assert got[1].any()
            back, wback = eng.subgraph_pool_bwd(operand, got[2], by=by, bf16=keyword, want64=True), eng.subgraph_pool_bwd(wide, got[2], by=by, want64=True)
            _eq(back[0], wback[0], f"{kind} {by} backward out32")
            _eq(back[1], wback[1], f"{kind} {by} backward out64")
    finally:
        eng.reset_options()


def test_refusals_a_subgraph_without_edges_and_what_the_calls_leave_alone(crafted, ref):
    eng, lib, d = crafted.eng, crafted.eng._lib, 3
    X = np.ascontiguousarray(ref["X"]["ties"][:, :d])
    row_ptr, cols, sub_ptr, sub_col, sub_eid, _ = eng.store_take_subgraph([0, 0], want_eid=True)
    gen, timing = eng.get_option("sparse_generation"), eng.timing()
    out, arg = np.full((NC, d), np.nan, dtype=np.float32), np.full((NC, d), 77, dtype=np.int32)
    fwd = lambda flags=0, ldx=d, a=arg: lib.fora_hip_subgraph_pool(eng._ctx, _p(X), 0, d, ldx, flags, _p(out), None, d, _p(a), d, None, None)
    bwd = lambda flags=0, ldx=d, a=arg: lib.fora_hip_subgraph_pool_bwd(eng._ctx, _p(X), 0, d, ldx, flags, _p(a), d, _p(out), None, d, None, None)
    # ---- refusals that write nothing: flag bit 1 (FORA_SUB_MEAN), a pitch below d, a NULL arg backward
    assert fwd(flags=1) == E_ARG and bwd(flags=1) == E_ARG and fwd(ldx=d - 1) == E_ARG and bwd(ldx=d - 1) == E_ARG and bwd(a=None) == E_ARG
    assert np.isnan(out).all() and (arg == 77).all()
    # ---- the calls leave the held result and the subgraph as they were
    for by in ("row", "col"):
        eng.subgraph_pool_bwd(X, eng.subgraph_pool(X, by=by)[2], by=by)
    assert eng.get_option("sparse_generation") == gen and eng.timing() == timing and eng.held_cols == NC
    for a, b, name in zip(eng.sparse_subgraph(row_ptr, want_eid=True)[:3], (sub_ptr, sub_col, sub_eid), ("sub_ptr", "sub_col", "sub_eid")):
        _eq(a, b, name)
    # ---- a subgraph of 0 edges: +0.0 and -1 forward, +0.0 backward
    crafted.take(row=1)
    assert eng.get_option("sub_edges") == 0 and eng.held_cols == 2
    for by in ("row", "col"):
        o32, o64, a, _ = eng.subgraph_pool(X[:2], by=by, out32=np.full((2, d), np.nan, np.float32), out64=np.full((2, d), np.nan), arg=np.full((2, d), 77, np.int32))
        assert not o32.any() and not o64.any() and not np.signbit(o64).any() and (a == -1).all()
        o32, o64, _ = eng.subgraph_pool_bwd(X[:2], a, by=by, out32=np.full((2, d), np.nan, np.float32), out64=np.full((2, d), np.nan))
        assert not o32.any() and not o64.any() and not np.signbit(o64).any()
    # ---- no subgraph held
    eng.store_take_compact([0, 0])
    assert eng.get_option("sub_edges") == -1 and fwd() == E_ARG and bwd() == E_ARG and np.isnan(out).all() and (arg == 77).all()
    with pytest.raises(Exception):
        eng.subgraph_pool(X)


def test_device_tensors_and_autograd():
    """Engine.subgraph_pool over device tensors and torch_ops.subgraph_pool, in a child of their own (tests/subgraph_pool_device_child.py):
    torch and the library must live on one HIP runtime, so the child imports torch first."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "subgraph_pool_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "subgraph pool device ok" in r.stdout
