"""EDGE SCORES on the GPU, through the C ABI (the contract of include/fora_hip_edge.h): score[h][e] over the held subgraph is the
numpy twin's (tests/subgraph_sddmm_ref.py) bit for bit for every group width, head count and element type; one call for all
heads equals the per-head calls on column slices; the call leaves the held result and the subgraph as they were -- every
comparison here is an equality of bits.  Memory of another GPU needs a second device and is not exercised here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import narrow_ref
import propagate_ref as pr
import propagate_values_ref as pv
import subgraph_prop_ref as sr
import subgraph_sddmm_ref as ss
from conftest import pick_sources
from test_sparse_gpu import _load
from test_subgraph_prop_gpu import Crafted, _eq, _p

pytestmark = pytest.mark.gpu
E_ARG = -1
WIDTH, PITCH = 130, 133
# every G from 1 to 64, a slice longer than 64, a head count that is no power of two, several heads per wave
SHAPES = [(1, 1), (1, 3), (1, 33), (1, 64), (1, 130), (2, 8), (3, 5), (4, 16), (8, 8), (2, 65)]


@pytest.fixture(scope="module")
def crafted():
    c = Crafted()
    yield c
    c.eng.close()


@pytest.fixture(scope="module")
def operands(crafted):
    """A and B [nc, 130] at pitch 133 with NaN padding, all values different and scaled over 2^+-20; the rows of A that belong
    to rows without edges are NaN and must never be read"""
    rng = np.random.Generator(np.random.PCG64(9960))
    out = {name: np.full((sr.CRAFTED_NC, PITCH), np.nan, dtype=np.float32) for name in ("A", "B")}
    for wide in out.values():
        wide[:, :WIDTH] = pv.distinct_values(rng, sr.CRAFTED_NC * WIDTH, np.float32).reshape(sr.CRAFTED_NC, WIDTH)
    out["A"][np.diff(crafted.sub[0]) == 0] = np.nan
    return out


@pytest.mark.parametrize("heads,d", SHAPES)
def test_against_the_twin_and_the_per_head_calls(crafted, operands, heads, d):
    eng, (sub_ptr, sub_col, _, _) = crafted.eng, crafted.sub
    crafted.take()
    A, B = operands["A"][:, :heads * d], operands["B"][:, :heads * d]
    w64, w32 = ss.scores(sub_ptr, sub_col, A, B, heads=heads)
    o32, o64, st = eng.subgraph_sddmm(A, B, heads=heads, want32=True, want64=True)
    _eq(o64, w64, "out64")
    _eq(o32, w32, "out32")
    assert not np.isnan(o64).any()                                                   # no row of A without edges, no padding was read
    assert st["edges"] == sub_col.size and st["workgroups"] == -(-(-(-sub_col.size // 64)) // 4) and st["a_on_device"] == st["b_on_device"] == 0
    for h in range(heads):
        one = eng.subgraph_sddmm(A[:, h * d:(h + 1) * d], B[:, h * d:(h + 1) * d], want32=False, want64=True)[1]
        _eq(one[0], o64[h], f"head {h} alone")


@pytest.mark.parametrize("heads,d", [(2, 8), (1, 33)])
@pytest.mark.parametrize("kind", ["bf16", narrow_ref.F16, narrow_ref.E4M3, narrow_ref.E5M2])
def test_narrow_operands_on_either_side_against_the_widened_f32_call(crafted, operands, kind, heads, d):
    eng = crafted.eng
    crafted.take()
    rng = np.random.Generator(np.random.PCG64(9961))
    shape = (sr.CRAFTED_NC, heads * d)
    if kind == "bf16":
        codes = pr.to_bf16_bits(pv.distinct_values(rng, shape[0] * shape[1], np.float32).reshape(shape))
        operand, keyword = codes, True
    else:
        codes = narrow_ref.moderate_codes(rng, kind, shape)
        operand, keyword = narrow_ref.as_operand(kind, codes)
    wide, other = sr.widen32(codes, kind), operands["B"][:, :heads * d]
    pairs = {"a": (eng.subgraph_sddmm(operand, other, heads=heads, want64=True, a_bf16=keyword), eng.subgraph_sddmm(wide, other, heads=heads, want64=True)),
             "b": (eng.subgraph_sddmm(other, operand, heads=heads, want64=True, b_bf16=keyword), eng.subgraph_sddmm(other, wide, heads=heads, want64=True))}
    for side, (got, ref) in pairs.items():
        _eq(got[0], ref[0], f"{kind} as {side}: out32")
        _eq(got[1], ref[1], f"{kind} as {side}: out64")
        assert got[1].any()
    both = eng.subgraph_sddmm(operand, operand, heads=heads, want64=True, a_bf16=keyword, b_bf16=keyword)[1]
    _eq(both, ss.scores(crafted.sub[0], crafted.sub[1], codes, codes, heads=heads, a_kind=kind, b_kind=kind)[0], f"{kind} on both sides")


def test_refusals_write_nothing_and_the_call_leaves_the_state_alone(crafted, operands):
    eng, fn = crafted.eng, crafted.eng._lib.fora_hip_subgraph_sddmm
    row_ptr, cols, sub_ptr, sub_col, sub_eid, _ = eng.store_take_subgraph([0, 0], want_eid=True)
    heads, d = 2, 3
    A, B = np.ascontiguousarray(operands["A"][:, :6]), np.ascontiguousarray(operands["B"][:, :6])
    out = np.full(heads * sub_col.size, np.nan, dtype=np.float32)

    def raw(ctx=eng._ctx, at=0, bt=0, lda=6, ldb=6, dd=d, hh=heads, o32=out, cap=out.size):
        return fn(ctx, _p(A), at, lda, _p(B), bt, ldb, dd, hh, _p(o32), None, cap, None, None)

    for bad in (dict(at=3), dict(bt=7), dict(dd=0), dict(hh=0), dict(lda=5), dict(ldb=5), dict(o32=None), dict(cap=out.size - 1),
                dict(dd=65536, hh=2, lda=1 << 17, ldb=1 << 17), dict(ctx=None)):
        assert raw(**bad) == E_ARG, bad
    assert np.isnan(out).all()
    # ---- the call leaves the held result, both transpositions and the subgraph as they were
    G = np.ones((2, d), dtype=np.float32)
    assert eng.sparse_propagate_t(row_ptr, G)[2]["built"] == 1 and eng.subgraph_propagate_t(A)[2]["built"] == 1
    e = int(row_ptr[-1])
    held = [np.zeros(e, np.int32), np.zeros(e, np.uint64), np.zeros(e, np.int32), np.zeros(e, np.uint64)]
    eng.sparse_fetch(held[0], None, held[1], cap=e)
    gen, timing = eng.get_option("sparse_generation"), eng.timing()
    assert raw() == 0 and not np.isnan(out).any()
    eng.subgraph_sddmm(A, B, heads=3, want64=True)
    assert eng.get_option("sparse_generation") == gen and eng.timing() == timing and eng.held_cols == sr.CRAFTED_NC
    eng.sparse_fetch(held[2], None, held[3], cap=e)
    _eq(held[2], held[0], "held ids")
    _eq(held[3], held[1], "held words")
    assert eng.sparse_propagate_t(row_ptr, G)[2]["built"] == 0 and eng.subgraph_propagate_t(A)[2]["built"] == 0
    for a, b, name in zip(eng.sparse_subgraph(row_ptr, want_eid=True)[:3], (sub_ptr, sub_col, sub_eid), ("sub_ptr", "sub_col", "sub_eid")):
        _eq(a, b, name)
    # ---- a subgraph of 0 edges (store row 1: two nodes): FORA_OK, nothing written; then no subgraph held
    crafted.take(row=1)
    out[:] = np.nan
    assert eng.get_option("sub_edges") == 0 and eng.held_cols == 2 and raw() == 0 and np.isnan(out).all()
    o32, o64, st = eng.subgraph_sddmm(A[:2], B[:2], heads=heads, want64=True)
    assert o32.shape == o64.shape == (heads, 0) and st["edges"] == 0 and st["workgroups"] == 0
    eng.store_take_compact([0, 0])
    assert raw() == E_ARG and np.isnan(out).all()
    with pytest.raises(Exception):
        eng.subgraph_sddmm(A, B)


def test_a_result_without_columns(engine, small):
    _load(engine, small, epsilon=0.5)
    rp0 = engine.query_sparse(pick_sources(small, 2, 9962), threshold=1.0)[0]
    assert int(rp0[-1]) == 0 and engine.sparse_compact(rp0)[0].size == 0 and engine.sparse_subgraph(rp0)[3]["edges"] == 0
    o32, o64, st = engine.subgraph_sddmm(np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), heads=2, want64=True)
    assert o32.shape == o64.shape == (2, 0) and st["workgroups"] == 0                # nc = 0: FORA_OK, nothing launched
    engine.sparse_clear()


def test_device_tensors_and_autograd():
    """the torch part in a child of its own (tests/subgraph_sddmm_device_child.py): torch and the library on one HIP runtime"""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "subgraph_sddmm_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0 and "subgraph sddmm device ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
