"""NARROW OPERANDS on the GPU, through the C ABI (the contract of include/fora_hip.h): with a dense operand in f16, FP8 E4M3 or FP8
E5M2 every call on the held rows gives, bit for bit, what it gives with that operand widened to float32 by the contract's rule
(tests/narrow_ref.py restates it with integers and ldexp).  Every comparison here is an equality of bits; where a NaN is
involved, NaN-ness is what agrees.  The first two tests run every code of every type through the vector-load and through the
one-element-per-lane load sites: they are what shows that the conversions the kernels use agree with the rule."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import narrow_ref as nr
import propagate_values_ref as pv
import sddmm_ref as sr
from conftest import pick_sources
from test_sparse_gpu import _load

pytestmark = pytest.mark.gpu
E_ARG = -1
F32, BF16 = "f32", "bf16"
N = 2000


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _same(got, want, name):
    """equal shapes, dtypes and bits; NaN compared in NaN-ness"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, name
    if got.dtype.kind != "f":
        assert (got == want).all(), name
        return
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), name
    u = {4: np.uint32, 8: np.uint64}[got.itemsize]
    assert (got.view(u)[~nan] == want.view(u)[~nan]).all(), name


def _bf16_bits(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _operand(kind, codes, wide):
    """(array, keyword): the operand as its own type, or (wide) as the float32 array of its widening"""
    if kind == F32:
        return np.ascontiguousarray(codes, dtype=np.float32), False
    if kind == BF16:
        codes = np.ascontiguousarray(codes, dtype=np.uint16)
        return ((codes.astype(np.uint32) << 16).view(np.float32), False) if wide else (codes, True)
    return (nr.widen(kind, codes), False) if wide else nr.as_operand(kind, codes)


def _draw(rng, kind, shape):
    if kind == F32:
        return rng.standard_normal(shape).astype(np.float32)
    if kind == BF16:
        return _bf16_bits(rng.standard_normal(shape))
    return nr.moderate_codes(rng, kind, shape)


@pytest.fixture(scope="module")
def identity_rows():
    """2000 rows, row i = {i}"""
    return np.arange(N + 1, dtype=np.int64), np.arange(N, dtype=np.int32), np.full(N, 1 << 40, dtype=np.uint64)


def _hold_identity(engine, g, identity_rows):
    assert g.n == N
    _load(engine, g, epsilon=0.5)
    engine.store_load(*identity_rows)
    row_ptr, _ = engine.store_take(np.arange(N))
    return row_ptr


def _every_code(kind, d):
    mask = 0xFFFF if kind == nr.F16 else 0xFF
    return ((np.arange(N * d, dtype=np.int64) & mask).reshape(N, d)).astype(nr.CODE_DTYPE[kind])


# (type, d, pitch): pitch 40 takes f16's widest load and pitch 33 its width 1; pitch 16 takes FP8's widest load and pitch 5 its
# width 1; the last three are d columns of a wider array, where the last lane of a row reads a tail of 5, 5 and 3 columns
VECTOR_CASES = [(nr.F16, 40, 40), (nr.F16, 33, 33), (nr.E4M3, 16, 16), (nr.E4M3, 5, 5), (nr.E5M2, 16, 16), (nr.E5M2, 5, 5),
                (nr.F16, 37, 40), (nr.E4M3, 21, 32), (nr.E5M2, 7, 8)]


@pytest.mark.parametrize("kind,d,pitch", VECTOR_CASES)
def test_every_code_through_the_vector_loads(engine, tiny, identity_rows, kind, d, pitch):
    """out[i][c] = 1.0 * H[i][c] over 2000 rows that hold every code of the type"""
    row_ptr = _hold_identity(engine, tiny, identity_rows)
    codes = np.full((N, pitch), 0x7E01 if kind == nr.F16 else 0x7F, dtype=nr.CODE_DTYPE[kind])     # (the padding: NaN codes, never read)
    codes[:, :d] = _every_code(kind, d)
    assert np.unique(codes[:, :d]).size == (65536 if kind == nr.F16 else 256)
    ones = np.ones(N, dtype=np.float64)
    H, kw = nr.as_operand(kind, codes)
    H, wide = H[:, :d], nr.widen(kind, codes)[:, :d]
    got32, got64, st = engine.sparse_propagate(row_ptr, H, want32=True, want64=True, bf16=kw, values=ones)
    want32, want64, wst = engine.sparse_propagate(row_ptr, wide, want32=True, want64=True, values=ones)
    _same(got64, want64, "out64 against the widened call")
    _same(got32, want32, "out32 against the widened call")
    ref64, ref32 = pv.propagate_vals_ref(row_ptr, identity_rows[1], ones, wide)
    _same(got64, ref64, "out64 against the twin")
    _same(got32, ref32, "out32 against the twin")
    _same(got32, wide + np.float32(0), "+0.0 + 1.0 * h is h, and +0.0 for -0.0")
    assert st["feat_bytes"] == N * d * H.itemsize and wst["feat_bytes"] == N * d * 4


@pytest.mark.parametrize("kind", [nr.F16, nr.E4M3, nr.E5M2])
def test_every_code_through_the_scalar_loads(engine, tiny, identity_rows, kind):
    """SDDMM reads one element per lane: every finite code as B against a random float32 A, then as A against a float32 B"""
    row_ptr = _hold_identity(engine, tiny, identity_rows)
    d = 33
    codes = _every_code(kind, d)
    codes = np.where(nr.is_finite_code(kind, codes), codes, 0).astype(codes.dtype)
    assert np.unique(codes).size >= (65536 - 2048 if kind == nr.F16 else 256 - 8)
    other = np.random.Generator(np.random.PCG64(9710)).standard_normal((N, d)).astype(np.float32)
    X, kw = nr.as_operand(kind, codes)
    wide = nr.widen(kind, codes)
    for name, a, b, akw, bkw, wa, wb in (("b narrow", other, X, False, kw, other, wide), ("a narrow", X, other, kw, False, wide, other)):
        got32, got64, st = engine.sparse_sddmm(row_ptr, a, b, want32=True, want64=True, a_bf16=akw, b_bf16=bkw)
        want32, want64, _ = engine.sparse_sddmm(row_ptr, wa, wb, want32=True, want64=True)
        _same(got64, want64, name + ": out64 against the widened call")
        _same(got32, want32, name + ": out32 against the widened call")
        ref64, ref32 = sr.sddmm_ref(row_ptr, identity_rows[1], wa, wb)
        _same(got64, ref64, name + ": out64 against the twin")
        _same(got32, ref32, name + ": out32 against the twin")
        assert st["bytes"] == N * d * (4 + X.itemsize)


# ---- every call, every new type, on rows that cross the kernels' edges
LENS = [0, 1, 63, 64, 65, 256, 257, 300]
HEADS, D, DV, DP = 2, 8, 6, 48
SDDMM_PAIRS = [(nr.F16, nr.E4M3), (nr.E5M2, BF16), (F32, nr.F16), (nr.E4M3, nr.E4M3)]
ATTN_TYPES = [(nr.F16, nr.E4M3, nr.E5M2, nr.F16), (F32, nr.F16, nr.E4M3, nr.E5M2)]      # q, k, v and the backward pass's g


def _crafted_rows(n, lens, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = [np.sort(rng.choice(n, size=L, replace=False)) for L in lens]
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate(rows).astype(np.int32)
    return row_ptr, ids, rng.integers(1, 1 << 50, size=ids.size, dtype=np.uint64)


def _all_calls(engine, row_ptr, n, wide, y_from=None):
    """every call with every new type; wide: the operands as their float32 widenings.  The codes depend on the seed alone, so
    the two runs read the same values.  Returns {name: array}"""
    rng = np.random.Generator(np.random.PCG64(9720))
    nq, e = len(row_ptr) - 1, int(row_ptr[-1])
    out = {}
    values = rng.standard_normal(e)
    for kind in (nr.F16, nr.E4M3, nr.E5M2):
        H, hk = _operand(kind, _draw(rng, kind, (n, DP)), wide)
        G, gk = _operand(kind, _draw(rng, kind, (nq, DP)), wide)
        for tag, kw in (("plain", {}), ("norm", {"normalize": True}), ("values", {"values": values})):
            o32, o64, st = engine.sparse_propagate(row_ptr, H, want32=True, want64=True, bf16=hk, **kw)
            out[f"prop {kind} {tag} 32"], out[f"prop {kind} {tag} 64"] = o32, o64
            assert st["feat_bytes"] == e * DP * H.itemsize
            o32, o64, st = engine.sparse_propagate_t(row_ptr, G, want32=True, want64=True, bf16=gk, **kw)
            out[f"prop_t {kind} {tag} 32"], out[f"prop_t {kind} {tag} 64"] = o32, o64
            assert st["feat_bytes"] == e * DP * G.itemsize
    for ak, bk in SDDMM_PAIRS:
        A, akw = _operand(ak, _draw(rng, ak, (nq, DP)), wide)
        B, bkw = _operand(bk, _draw(rng, bk, (n, DP)), wide)
        o32, o64, st = engine.sparse_sddmm(row_ptr, A, B, want32=True, want64=True, a_bf16=akw, b_bf16=bkw)
        out[f"sddmm {ak} {bk} 32"], out[f"sddmm {ak} {bk} 64"] = o32, o64
        assert st["bytes"] == e * DP * (A.itemsize + B.itemsize)
    for qk, kk, vk, gk in ATTN_TYPES:
        tag = f"{qk} {kk} {vk}"
        Q, qw = _operand(qk, _draw(rng, qk, (nq, HEADS * D)), wide)
        K, kw = _operand(kk, _draw(rng, kk, (n, HEADS * D)), wide)
        V, vw = _operand(vk, _draw(rng, vk, (n, HEADS * DV)), wide)
        G, gw = _operand(gk, _draw(rng, gk, (nq, HEADS * DV)), wide)
        o32, o64, y32, y64, st = engine.sparse_attention(row_ptr, Q, K, V, heads=HEADS, want32=True, want64=True, want_y32=True, want_y64=True,
                                                         q_bf16=qw, k_bf16=kw, v_bf16=vw)
        assert st["nan_rows"] == 0
        out[f"attn {tag} 32"], out[f"attn {tag} 64"], out[f"attn {tag} y32"], out[f"attn {tag} y64"] = o32, o64, y32, y64
        out[f"attn {tag} split"] = np.array([st["short_rows"], st["long_rows"]])
        y = y64 if y_from is None else y_from[f"attn {tag} y64"]
        grads = engine.sparse_attention_bwd(row_ptr, Q, K, V, G, y, heads=HEADS, want32=True, want64=True, q_bf16=qw, k_bf16=kw, v_bf16=vw, g_bf16=gw)
        for name, g in zip(("dq32", "dq64", "dk32", "dk64", "dv32", "dv64"), grads[:6]):
            out[f"bwd {tag} g {gk} {name}"] = g
    return out


def _compare_all(engine, row_ptr, n, want_long):
    wide = _all_calls(engine, row_ptr, n, True)
    narrow = _all_calls(engine, row_ptr, n, False, y_from=wide)
    assert wide.keys() == narrow.keys() and len(wide) > 60
    for name in wide:
        _same(narrow[name], wide[name], name)
    for name in wide:
        if name.endswith("split"):
            short, lng = wide[name]
            assert (lng >= 1) if want_long else (short >= 1), name
        elif wide[name].dtype.kind == "f":
            assert np.abs(np.nan_to_num(wide[name])).sum() > 0, name          # (the call computed something)


@pytest.mark.parametrize("long_paths", [False, True])
def test_every_call_on_crafted_rows(engine, tiny, long_paths):
    """rows of 0, 1, 63, 64, 65, 256, 257 and 300 entries; long_paths: attn_short = 0 and propt_lds_cap = 0, so that every row and
    column takes the longer rows' kernels and the transposition's global tier"""
    g = tiny
    assert g.n == N
    _load(engine, g, epsilon=0.5)
    engine.store_load(*_crafted_rows(N, LENS, 9721))
    try:
        if long_paths:
            engine.set_option("attn_short", 0)
            engine.set_option("propt_lds_cap", 0)
        row_ptr, _ = engine.store_take(np.arange(len(LENS)))
        assert np.diff(row_ptr).tolist() == LENS
        _compare_all(engine, row_ptr, N, want_long=True)
    finally:
        engine.reset_options()


@pytest.mark.parametrize("long_paths", [False, True])
def test_every_call_on_a_topk_result(engine, tiny_dangling, long_paths):
    g = tiny_dangling
    _load(engine, g, epsilon=0.5)
    srcs = np.concatenate([pick_sources(g, 6, 9722), pick_sources(g, 1, 9723, want_dangling=True)])
    try:
        if long_paths:
            engine.set_option("attn_short", 0)
            engine.set_option("propt_lds_cap", 0)
        row_ptr = engine.query_sparse_topk(srcs, 16, threshold=0.0)[0]
        assert int(row_ptr[-1]) > 16
        _compare_all(engine, row_ptr, g.n, want_long=long_paths)
    finally:
        engine.reset_options()


def test_compacted(engine, tiny):
    """after sparse_compact the operands are X[cols]: propagate and attention in E4M3 equal the widened calls"""
    g = tiny
    _load(engine, g, epsilon=0.5)
    engine.store_load(*_crafted_rows(N, [5, 0, 64, 130, 300], 9730))
    row_ptr, _ = engine.store_take(np.arange(5))
    cols, _ = engine.sparse_compact(row_ptr)
    nq, nc = 5, cols.size
    assert 300 <= nc < N and engine.held_cols == nc
    rng = np.random.Generator(np.random.PCG64(9731))
    Hc = nr.moderate_codes(rng, nr.E4M3, (N, DP))[cols]
    Kc = nr.moderate_codes(rng, nr.E4M3, (N, HEADS * D))[cols]
    Vc = nr.moderate_codes(rng, nr.E4M3, (N, HEADS * DV))[cols]
    Q = rng.standard_normal((nq, HEADS * D)).astype(np.float32)
    got = engine.sparse_propagate(row_ptr, np.ascontiguousarray(Hc), want32=True, want64=True, bf16="e4m3")
    want = engine.sparse_propagate(row_ptr, nr.widen(nr.E4M3, Hc), want32=True, want64=True)
    _same(got[0], want[0], "propagate 32")
    _same(got[1], want[1], "propagate 64")
    got = engine.sparse_attention(row_ptr, Q, np.ascontiguousarray(Kc), np.ascontiguousarray(Vc), heads=HEADS, want32=True, want64=True, want_y64=True,
                                  k_bf16="e4m3", v_bf16="e4m3")
    want = engine.sparse_attention(row_ptr, Q, nr.widen(nr.E4M3, Kc), nr.widen(nr.E4M3, Vc), heads=HEADS, want32=True, want64=True, want_y64=True)
    for i, name in ((0, "attention 32"), (1, "attention 64"), (3, "attention y64")):
        _same(got[i], want[i], name)
    assert np.abs(want[1]).sum() > 0
    with pytest.raises(ValueError):                        # (an operand over all n nodes is refused by the binding)
        engine.sparse_propagate(row_ptr, np.zeros((N, DP), np.uint8), bf16="e4m3")


def test_alignment_device_memory_and_autograd():
    """torch tensors of the three dtypes on the GPU, contiguous and as column slices at odd and even pitches, and the torch_ops
    functions, in a child of their own (tests/narrow_device_child.py): torch and the library must live on one HIP runtime, so the
    child imports torch first."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "narrow_device_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "narrow device ok" in r.stdout


# ---- refusals
def test_refusals(engine, tiny):
    g = tiny
    _load(engine, g, epsilon=0.5)
    engine.store_load(*_crafted_rows(N, [3, 0, 70], 9740))
    row_ptr, _ = engine.store_take(np.arange(3))
    nq, e = 3, int(row_ptr[-1])
    lib, ctx = engine._lib, engine._ctx
    d, dv, heads = 4, 4, 1
    feat = np.zeros((N, 8), np.float32)            # room for every type at these shapes
    rows = np.zeros((nq, 8), np.float32)
    per = np.full(e, 0.25, np.float64)
    SENT = 12345.0
    o32, o64 = np.full((N, 8), SENT, np.float32), np.full((N, 8), SENT, np.float64)
    e32, e64 = np.full(e, SENT, np.float32), np.full(e, SENT, np.float64)
    from fora_amd import capi
    gr = capi.AttnGrads()
    gr.dq32, gr.lddq = _p(o32).value, 8
    i, i64, u64, dbl = C.c_int, C.c_int64, C.c_uint64, C.c_double
    rp = _p(row_ptr)

    def prop(ft, vals=None, vt=0):
        if vals is None:
            return lib.fora_hip_sparse_propagate(ctx, rp, i(nq), _p(feat), i(ft), i(d), i64(8), i(0), _p(o32), _p(o64), i64(8), None)
        return lib.fora_hip_sparse_propagate_vals(ctx, rp, i(nq), _p(feat), i(ft), i(d), i64(8), i(0), _p(vals), i(vt), _p(o32), _p(o64), i64(8), None)

    def prop_t(gt, vals=None, vt=0):
        if vals is None:
            return lib.fora_hip_sparse_propagate_t(ctx, rp, i(nq), _p(rows), i(gt), i(d), i64(8), i(0), _p(o32), _p(o64), i64(8), None)
        return lib.fora_hip_sparse_propagate_t_vals(ctx, rp, i(nq), _p(rows), i(gt), i(d), i64(8), i(0), _p(vals), i(vt), _p(o32), _p(o64), i64(8), None)

    def sddmm(at, bt):
        return lib.fora_hip_sparse_sddmm(ctx, rp, i(nq), _p(rows), i(at), i64(8), _p(feat), i(bt), i64(8), i(d), _p(e32), _p(e64), u64(e), None)

    def attn(qt, kt, vt):
        return lib.fora_hip_sparse_attention(ctx, rp, i(nq), _p(rows), i(qt), i64(8), _p(feat), i(kt), i64(8), _p(feat), i(vt), i64(8), i(d), i(dv), i(heads),
                                             dbl(0.5), _p(o32), _p(o64), i64(8), _p(e32), _p(e64), u64(e), None)

    def bwd(qt, kt, vt, gt, yt=2):
        return lib.fora_hip_sparse_attention_bwd(ctx, rp, i(nq), _p(rows), i(qt), i64(8), _p(feat), i(kt), i64(8), _p(feat), i(vt), i64(8), _p(rows), i(gt), i64(8),
                                                 _p(per), i(yt), u64(e), i(d), i(dv), i(heads), dbl(0.5), C.byref(gr), None)

    def softmax(t):
        return lib.fora_hip_sparse_softmax(ctx, rp, i(nq), _p(per), i(t), dbl(1.0), _p(e32), _p(e64), u64(e), None)

    def softmax_bwd(yt, gt):
        return lib.fora_hip_sparse_softmax_bwd(ctx, rp, i(nq), _p(per), i(yt), _p(per), i(gt), dbl(1.0), _p(e32), _p(e64), u64(e), None)

    calls = []
    for bad in (3, 7):                                     # no type: in every operand slot
        calls += [lambda b=bad: prop(b), lambda b=bad: prop(b, per, 2), lambda b=bad: prop_t(b), lambda b=bad: prop_t(b, per, 2),
                  lambda b=bad: sddmm(b, 0), lambda b=bad: sddmm(0, b),
                  lambda b=bad: attn(b, 0, 0), lambda b=bad: attn(0, b, 0), lambda b=bad: attn(0, 0, b),
                  lambda b=bad: bwd(b, 0, 0, 0), lambda b=bad: bwd(0, b, 0, 0), lambda b=bad: bwd(0, 0, b, 0), lambda b=bad: bwd(0, 0, 0, b)]
    for t in (4, 5, 6):                                    # a narrow type where bf16 is refused too
        calls += [lambda t=t: prop(0, per, t), lambda t=t: prop_t(0, per, t), lambda t=t: softmax(t), lambda t=t: softmax_bwd(t, 0),
                  lambda t=t: softmax_bwd(0, t), lambda t=t: bwd(0, 0, 0, 0, yt=t)]
    for k, call in enumerate(calls):
        assert call() == E_ARG, k
    for a in (o32, o64, e32, e64):
        assert (a == SENT).all()                           # nothing written
    assert prop(4) == 0 and prop_t(6) == 0 and sddmm(5, 6) == 0 and attn(4, 5, 6) == 0 and bwd(4, 5, 6, 4) == 0     # (the slots take the types)
    # the binding
    H8 = np.zeros((N, 4), np.uint8)
    with pytest.raises(ValueError):
        engine.sparse_propagate(row_ptr, H8)                                   # uint8 without the keyword
    with pytest.raises(ValueError):
        engine.sparse_propagate(row_ptr, H8, bf16=True)                        # uint8 is not bf16
    with pytest.raises(ValueError):
        engine.sparse_propagate(row_ptr, H8.astype(np.uint16), bf16="e4m3")    # uint16 is not FP8
    with pytest.raises(ValueError):
        engine.sparse_propagate(row_ptr, H8, bf16="e4m3fnuz")
    with pytest.raises(ValueError):
        engine.sparse_propagate(row_ptr, np.zeros((N, 4), np.float64))
    with pytest.raises(ValueError):
        engine.sparse_sddmm(row_ptr, np.zeros((nq, 4), np.float32), np.zeros((N, 4), np.float64))
    half = np.full(e, 0.25, np.float16)
    with pytest.raises(ValueError):
        engine.sparse_propagate(row_ptr, feat, values=half)
    with pytest.raises(ValueError):
        engine.sparse_softmax(row_ptr, half)
    with pytest.raises(ValueError):
        engine.sparse_softmax_bwd(row_ptr, per, half)
    with pytest.raises(ValueError):
        engine.sparse_attention_bwd(row_ptr, rows[:, :4], feat[:, :4], feat[:, :4], rows[:, :4], half.reshape(1, e))
    assert engine.sparse_propagate(row_ptr, H8, bf16="e5m2")[0].shape == (nq, 4)
    assert engine.sparse_propagate(row_ptr, H8.astype(np.uint16), bf16="bf16")[0].shape == (nq, 4)   # "bf16" means what True means
    assert engine.sparse_propagate(row_ptr, np.zeros((N, 4), np.float16))[0].shape == (nq, 4)
