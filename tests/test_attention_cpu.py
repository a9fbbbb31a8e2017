"""ATTENTION (fora_hip_sparse_attention) without a GPU: the twin (tests/attention_ref.py) against its three steps and against a
plain float64 attention, the host-side split of the rows (fora_amd/csrc/fora_attn_plan.h) against brute force under the
sanitizers, and the ABI surface."""
import math
import os
import subprocess

import numpy as np
import pytest

import attention_ref as ar
import propagate_values_ref as pv
import sddmm_ref as sr
import softmax_ref as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LENS = [0, 1, 3, 64, 65, 256, 257, 600]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _row_ptr(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _case(seed, d, dv, heads, n=700, lens=LENS):
    rng = np.random.Generator(np.random.PCG64(seed))
    row_ptr = _row_ptr(lens)
    ids = np.concatenate([np.sort(rng.choice(n, size=L, replace=False)) for L in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    Q, K = ar.scores_operands(rng, len(lens), n, d, heads)
    V = (rng.standard_normal((n, heads * dv)) * np.exp2(rng.integers(-6, 7, size=(n, heads * dv)))).astype(np.float32)
    return row_ptr, ids, Q, K, V


def test_the_twin_is_the_composition_of_the_three_twins():
    d, dv, heads, scale = 5, 3, 2, 0.37
    row_ptr, ids, Q, K, V = _case(9700, d, dv, heads)
    out64, out32, y64, y32, nan_rows = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, scale)
    assert nan_rows == 0 and out64.shape == (len(LENS), heads * dv) and y64.shape == (heads, int(row_ptr[-1]))
    assert (out32.view(np.uint32) == out64.astype(np.float32).view(np.uint32)).all() and (y32.view(np.uint32) == y64.astype(np.float32).view(np.uint32)).all()
    for j in range(heads):
        s64, _ = sr.sddmm_ref(row_ptr, ids, Q[:, j * d:(j + 1) * d], K[:, j * d:(j + 1) * d])
        yj, _, _ = sm.softmax_ref(row_ptr, s64, scale)
        oj, _ = pv.propagate_vals_ref(row_ptr, ids, yj, V[:, j * dv:(j + 1) * dv])
        assert (_bits(y64[j]) == _bits(yj)).all() and (_bits(out64[:, j * dv:(j + 1) * dv]) == _bits(oj)).all()
    assert (_bits(out64[0]) == 0).all()                          # the empty row: +0.0
    # the f64 scores matter: rounding them to f32 in between changes bits of y
    _, s32 = sr.sddmm_ref(row_ptr, ids, Q[:, :d], K[:, :d])
    y_via32, _, _ = sm.softmax_ref(row_ptr, s32, scale)
    assert (_bits(y_via32) != _bits(y64[0])).any()


@pytest.mark.parametrize("bf16", [(False, False, False), (True, False, True), (False, True, False)])
def test_heads_equal_single_head_calls_on_column_slices(bf16):
    import propagate_ref as pr
    d, dv, heads, scale = 7, 4, 3, -2.0
    row_ptr, ids, Q, K, V = _case(9710, d, dv, heads, lens=[3, 0, 70, 300])
    qb, kb, vb = bf16
    Q, K, V = (pr.to_bf16_bits(X) if b else X for X, b in ((Q, qb), (K, kb), (V, vb)))
    out64, _, y64, _, _ = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, scale, qb, kb, vb)
    for j in range(heads):
        o1, _, y1, _, _ = ar.attention_ref(row_ptr, ids, Q[:, j * d:(j + 1) * d], K[:, j * d:(j + 1) * d], V[:, j * dv:(j + 1) * dv], d, dv, 1, scale, qb, kb, vb)
        assert (_bits(out64[:, j * dv:(j + 1) * dv]) == _bits(o1)).all() and (_bits(y64[j]) == _bits(y1[0])).all()


def test_nan_rows_are_written_and_counted_per_head():
    d, dv, heads = 4, 3, 2
    row_ptr, ids, Q, K, V = _case(9720, d, dv, heads, lens=[5, 0, 70, 300, 2])
    K = K.copy()
    K[ids[row_ptr[2] + 7], 1] = np.nan                           # head 0 of row 2 (and of any other row that keeps this id)
    K[ids[row_ptr[3] + 290], d + 2] = np.inf                     # head 1 of row 3
    hit = {(i, j) for i in range(5) for j, col_id in ((0, ids[row_ptr[2] + 7]), (1, ids[row_ptr[3] + 290]))
           if col_id in ids[row_ptr[i]:row_ptr[i + 1]]}
    out64, out32, y64, y32, nan_rows = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, 0.5)
    assert nan_rows == len(hit) >= 2
    for i in range(5):
        for j in range(heads):
            o, y = out64[i, j * dv:(j + 1) * dv], y64[j, row_ptr[i]:row_ptr[i + 1]]
            if (i, j) in hit:
                assert (_bits(o) == 0x7FF8000000000000).all() and (_bits(y) == 0x7FF8000000000000).all()
                assert (out32[i, j * dv:(j + 1) * dv].view(np.uint32) == 0x7FC00000).all()
            else:
                assert np.isfinite(o).all() and np.isfinite(y).all()
    # scale = 0 turns every score into +-0.0: uniform rows, y = 1 / len -- but a non-finite score becomes NaN
    out0, _, y0, _, n0 = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, 0.0)
    assert n0 == len(hit)
    for j in range(heads):
        if (0, j) not in hit:
            assert (_bits(y0[j, row_ptr[0]:row_ptr[1]]) == _bits(1.0 / 5.0)).all()


@pytest.mark.parametrize("d", [3, 64, 65])
def test_the_twin_is_within_the_bound_of_a_plain_f64_attention(d):
    """Against math.exp and math.fsum, per (row, head, column), the bound computed from the rounding counts of the three steps:
    scores   the products are exact; an entry's sum goes through at most ceil(d / 64) - 1 adds of a lane and 6 of the tree:
             |s - s_exact| <= (ceil(d / 64) + 6) u sum_c |q_c k_c|.  The reference's fsum is s_exact rounded once, x = s * scale
             rounds once on either side, t = x - m once on either side: the argument of exp differs by at most
             eta_e = |scale| (ceil(d / 64) + 6) u sum_c |q_c k_c| + 3 u |x_e| + 2 u |t_e|   (the maximum itself cancels: a softmax does
             not depend on what is subtracted).
    softmax  d log y_e = eps_e - sum_k y_k eps_k, so the arguments' errors change y_e by at most 2 max eta relatively; on equal
             arguments the twin is within (ceil(len / 256) + 16) u of the plain softmax (tests/test_softmax_cpu.py).
    product  each term rounds once on either side, the twin then adds at most len - 1 + ceil(len / 256) - 1 times, fsum rounds
             once: (len + ceil(len / 256) + 3) u sum_e y_e |h_ec|.
    The three add up on sum_e y_e |h_ec|; 1 % on top for the second-order terms.  Nothing is tuned on what the twin gives."""
    dv, heads = 5, 2
    row_ptr, ids, Q, K, V = _case(9730 + d, d, dv, heads)
    Q64, K64, V64 = Q.astype(np.float64), K.astype(np.float64), V.astype(np.float64)
    for scale in (0.37, -2.0):
        out64, _, y64, _, nan_rows = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, scale)
        assert nan_rows == 0
        worst = 0.0
        for i, L in enumerate(LENS):
            if not L:
                continue
            a, b = int(row_ptr[i]), int(row_ptr[i + 1])
            segs = -(-L // 256)
            for j in range(heads):
                q = Q64[i, j * d:(j + 1) * d]
                kk = K64[ids[a:b], j * d:(j + 1) * d]
                s = [math.fsum((q * kr).tolist()) for kr in kk]
                mass = [math.fsum(np.abs(q * kr).tolist()) for kr in kk]
                x = [v * scale for v in s]
                m = max(x)
                t = [v - m for v in x]
                p = [math.exp(v) for v in t]
                S = math.fsum(p)
                y = [v / S for v in p]
                eta = max(abs(scale) * (-(-d // 64) + 6) * U * ms + 3 * U * abs(xe) + 2 * U * abs(te) for ms, xe, te in zip(mass, x, t))
                rel = 1.01 * ((segs + 16) * U + 2 * eta + (L + segs + 3) * U)
                yerr = max(abs(float(y64[j, a + e]) - y[e]) / y[e] for e in range(L))
                assert yerr <= 1.01 * ((segs + 16) * U + 2 * eta), (L, j, yerr)
                for c in range(dv):
                    h = V64[ids[a:b], j * dv + c]
                    ref = math.fsum([ye * he for ye, he in zip(y, h.tolist())])
                    bound = rel * math.fsum([ye * abs(he) for ye, he in zip(y, h.tolist())])
                    err = abs(float(out64[i, j * dv + c]) - ref)
                    worst = max(worst, err / bound)
                    assert err <= bound, (L, j, c, err, bound)
        print(f"d={d} scale={scale}: worst error / bound = {worst:.3f}")


def test_stats_ref():
    st = ar.attention_stats_ref(_row_ptr(sm.ROW_LENS))
    assert st == {"entries": sum(sm.ROW_LENS), "segments": 1 * 7 + 2 + 3 + 1, "max_row": 600, "short_rows": 8, "long_rows": 2}
    assert ar.attention_stats_ref(_row_ptr(sm.ROW_LENS), 0)["long_rows"] == 10 and ar.attention_stats_ref(_row_ptr(sm.ROW_LENS), 64)["short_rows"] == 5


@pytest.fixture(scope="session")
def attn_plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attn_plan") / "attn_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "attn_plan_check.cpp")], check=True)
    return exe


def test_the_split_of_the_rows_against_brute_force(attn_plan_check):
    """fora_attn_plan.h: every row in exactly one list, every entry covered once, the longer rows' plan chunked as PROPAGATE's"""
    rng = np.random.Generator(np.random.PCG64(9740))
    cases = [[0, 1, 255, 256, 257, 600], [1, 0, 255, 0, 0, 256, 257, 0, 600, 0], [], [0, 0], [3, 64, 1, 256, 0, 17],     # (only short rows)
             [257, 600, 1000, 300], [1, 600, 1, 26140, 0, 64], [int(x) for x in rng.integers(0, 900, size=40)]]        # (only long rows at 256)
    for lens in cases:
        for option in (0, 1, 64, 256, 1000, -5):
            for per in (1, 2, 3, 1 << 20):
                arg = ",".join(map(str, lens)) or "-"
                r = subprocess.run([attn_plan_check, str(option), str(per), arg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                assert r.returncode == 0 and not r.stderr, (option, per, lens, r.stdout[-500:], r.stderr[-2000:])
                st = ar.attention_stats_ref(_row_ptr(lens), option)
                cap = min(max(option, 0), 256)
                long_segs = sum(-(-L // 256) for L in lens if L > cap)
                chunks = max(1, -(-long_segs // per)) if lens else 0
                assert r.stdout.split() == [f"short={sum(1 for L in lens if L <= cap)}", f"long_segs={long_segs}", f"short_rows={st['short_rows']}",
                                            f"long_rows={st['long_rows']}", f"chunks={chunks}", "ok"]


def test_abi_surface():
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    assert " * ATTENTION (fora_hip_sparse_attention)" in hdr and hdr.index("ROW SOFTMAX (") < hdr.index("ATTENTION (") < hdr.index("PROPAGATE WITH VALUES (")
    assert capi.STRUCTS["fora_attn_stats"] is capi.AttnStats  # (its fields and size against the header: tests/test_capi_cpu.py)
    product, test = capi.load(), capi.load(capi.TEST_LIB)
    name = "fora_hip_sparse_attention"
    assert hasattr(product, name) and hasattr(test, name) and name in capi.SYMBOLS
    # NULL ctx: answered without touching the GPU
    assert product.fora_hip_sparse_attention(None, None, 0, None, 0, 1, None, 0, 1, None, 0, 1, 1, 1, 1, 1.0, None, None, 1, None, None, 0, None) == -1
    assert callable(capi.Engine.sparse_attention)
    from fora_amd import torch_ops
    assert callable(torch_ops.ppr_attention_fused)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "attn_short" in doc
