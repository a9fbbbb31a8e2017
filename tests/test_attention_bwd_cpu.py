"""ATTENTION, BACKWARD (fora_hip_sparse_attention_bwd) without a GPU: the twin (tests/attention_bwd_ref.py) against its steps,
against single-head twins and against float64 torch autograd of the plain dense-masked attention; the host-side split of the
columns (fora_amd/csrc/fora_attn_bwd_plan.h) against brute force under the sanitizers; the ABI surface."""
import os
import subprocess

import numpy as np
import pytest

import attention_bwd_ref as abr
import attention_ref as ar
import propagate_values_ref as pv
import sddmm_ref as sr
import softmax_ref as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LENS = [0, 1, 3, 64, 65, 256, 257, 600]
N = 700


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _row_ptr(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _case(seed, d, dv, heads, n=N, lens=LENS):
    rng = np.random.Generator(np.random.PCG64(seed))
    row_ptr = _row_ptr(lens)
    ids = np.concatenate([np.sort(rng.choice(n, size=L, replace=False)) for L in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    Q, K = ar.scores_operands(rng, len(lens), n, d, heads)
    V = (rng.standard_normal((n, heads * dv)) * np.exp2(rng.integers(-6, 7, size=(n, heads * dv)))).astype(np.float32)
    G = (rng.standard_normal((len(lens), heads * dv)) * np.exp2(rng.integers(-6, 7, size=(len(lens), heads * dv)))).astype(np.float32)
    return row_ptr, ids, Q, K, V, G


def test_the_twin_is_the_composition_of_the_step_twins():
    d, dv, heads, scale = 5, 3, 2, 0.37
    row_ptr, ids, Q, K, V, G = _case(9900, d, dv, heads)
    _, _, y64, y32, _ = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, scale)
    for y in (y64, y32):
        dq, dk, dvv = abr.attention_bwd_ref(row_ptr, ids, Q, K, V, G, y, N, d, dv, heads, scale)
        assert dq.shape == (len(LENS), heads * d) and dk.shape == (N, heads * d) and dvv.shape == (N, heads * dv)
        for j in range(heads):
            qs, vs = slice(j * d, (j + 1) * d), slice(j * dv, (j + 1) * dv)
            dy, _ = sr.sddmm_ref(row_ptr, ids, G[:, vs], V[:, vs])
            ds, _ = sm.softmax_bwd_ref(row_ptr, y[j], dy, scale)
            assert (_bits(dq[:, qs]) == _bits(pv.propagate_vals_ref(row_ptr, ids, ds, K[:, qs])[0])).all()
            assert (_bits(dk[:, qs]) == _bits(pv.propagate_t_vals_ref(row_ptr, ids, ds, Q[:, qs], N)[0])).all()
            assert (_bits(dvv[:, vs]) == _bits(pv.propagate_t_vals_ref(row_ptr, ids, y[j], G[:, vs], N)[0])).all()
        assert (_bits(dq[0]) == 0).all()                              # the empty row: +0.0
        empty = np.setdiff1d(np.arange(N), ids)
        assert empty.size and (_bits(dk[empty]) == 0).all() and (_bits(dvv[empty]) == 0).all()      # columns with no entry: +0.0
    # the f64 dy matters: rounding it to f32 in between changes bits of ds
    dy64, dy32 = sr.sddmm_ref(row_ptr, ids, G[:, :dv], V[:, :dv])
    assert (_bits(sm.softmax_bwd_ref(row_ptr, y64[0], dy64, scale)[0]) != _bits(sm.softmax_bwd_ref(row_ptr, y64[0], dy32, scale)[0])).any()
    # and so does the type of y
    a = abr.attention_bwd_ref(row_ptr, ids, Q, K, V, G, y64, N, d, dv, heads, scale)
    b = abr.attention_bwd_ref(row_ptr, ids, Q, K, V, G, y32, N, d, dv, heads, scale)
    assert all((_bits(x) != _bits(z)).any() for x, z in zip(a, b))


@pytest.mark.parametrize("bf16", [(False, False, False, False), (True, False, True, False), (False, True, False, True)])
def test_heads_equal_single_head_twins_on_column_slices(bf16):
    import propagate_ref as pr
    d, dv, heads, scale = 7, 4, 3, -2.0
    row_ptr, ids, Q, K, V, G = _case(9910, d, dv, heads, lens=[3, 0, 70, 300])
    _, _, y64, _, _ = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, scale)
    qb, kb, vb, gb = bf16
    Q, K, V, G = (pr.to_bf16_bits(X) if b else X for X, b in ((Q, qb), (K, kb), (V, vb), (G, gb)))
    dq, dk, dvv = abr.attention_bwd_ref(row_ptr, ids, Q, K, V, G, y64, N, d, dv, heads, scale, qb, kb, vb, gb)
    for j in range(heads):
        qs, vs = slice(j * d, (j + 1) * d), slice(j * dv, (j + 1) * dv)
        q1, k1, v1 = abr.attention_bwd_ref(row_ptr, ids, Q[:, qs], K[:, qs], V[:, vs], G[:, vs], y64[j:j + 1], N, d, dv, 1, scale, qb, kb, vb, gb)
        assert (_bits(dq[:, qs]) == _bits(q1)).all() and (_bits(dk[:, qs]) == _bits(k1)).all() and (_bits(dvv[:, vs]) == _bits(v1)).all()


@pytest.mark.parametrize("d,dv", [(3, 5), (64, 64), (65, 130)])
def test_the_twin_is_within_the_bound_of_f64_autograd(d, dv):
    """Against torch autograd in float64 of out = softmax(mask(Q K^T scale)) V, loss = sum(out G), on the CPU.  Both sides round;
    the bound below holds for EITHER side against exact arithmetic, so the two differ by at most twice it.  u = 2^-53, a sum of
    m terms in any order errs by at most (m - 1) u sum |terms|, per (row, head) of L entries in segs = ceil(L / 256) segments:
    y       both sides are within rho = (segs + 16 + L + 4) u + 2 eta relatively: the twin's forward bound
            (tests/test_attention_cpu.py: (segs + 16) u + 2 eta) and a plain softmax's exp, L - 1 adds and division; eta_e =
            |scale| (d + 6) u sum_c |q_c k_c| + 3 u |x_e| + 2 u |t_e| bounds the error of exp's argument on both sides (the twin
            adds ceil(d / 64) + 6 times, a matmul at most d times).
    dy      exact products, at most ceil(dv / 64) + 6 adds in the twin and dv in a matmul: a_e = (dv + 6) u sum_c |g_c v_ec|.
    D       t_e = y_e dy_e rounds once, the twin adds at most 10 + segs times per term's path, a plain sum L - 1 times:
            eps_D = (L + segs + 12) u T + rho T + sum_e y_e a_e with T = sum_e y_e |dy_e|.
    ds      at most five roundings on either side: b_e = (5 u + rho) |ds_e| + |scale| y_e (a_e + eps_D).
    dq      each term rounds once, then at most L - 1 + segs adds: (L + segs + 2) u sum_e |ds_e k_ec| + sum_e b_e |k_ec|.
    dk, dv  the same over a column of Lc entries: (Lc + segs_c + 2) u sum |ds_e q_c| + sum b_e |q_c|, and
            (Lc + segs_c + 2) u sum y_e |g_c| + sum rho y_e |g_c|.
    1 % on top for the second-order terms.  Nothing is tuned on what the twin gives."""
    import torch
    heads = 2
    row_ptr, ids, Q, K, V, G = _case(9920 + d, d, dv, heads)
    nq, E = len(LENS), int(row_ptr[-1])
    er = sr.entry_rows(row_ptr)
    idl = ids.astype(np.int64)
    mask = np.zeros((nq, N), dtype=bool)
    mask[er, idl] = True
    col_len = np.bincount(idl, minlength=N)
    for scale in (0.37, -2.0):
        _, _, y64, _, nan_rows = ar.attention_ref(row_ptr, ids, Q, K, V, d, dv, heads, scale)
        assert nan_rows == 0
        dq, dk, dvv = abr.attention_bwd_ref(row_ptr, ids, Q, K, V, G, y64, N, d, dv, heads, scale)
        tq, tk, tv = (torch.tensor(X.astype(np.float64), requires_grad=True) for X in (Q, K, V))
        tm, tg = torch.tensor(mask), torch.tensor(G.astype(np.float64))
        outs = []
        for j in range(heads):
            s = (tq[:, j * d:(j + 1) * d] @ tk[:, j * d:(j + 1) * d].T) * scale
            p = torch.softmax(s.masked_fill(~tm, float("-inf")), dim=1)
            p = torch.where(tm, p, torch.zeros_like(p))              # (the empty row: nan -> 0)
            outs.append(p @ tv[:, j * dv:(j + 1) * dv])
        (torch.cat(outs, dim=1) * tg).sum().backward()
        rq, rk, rv = tq.grad.numpy(), tk.grad.numpy(), tv.grad.numpy()
        worst = {"dq": 0.0, "dk": 0.0, "dv": 0.0}
        Q64, K64, V64, G64 = (X.astype(np.float64) for X in (Q, K, V, G))
        for j in range(heads):
            qs, vs = slice(j * d, (j + 1) * d), slice(j * dv, (j + 1) * dv)
            qe, ke, ve, ge = Q64[er, qs], K64[idl, qs], V64[idl, vs], G64[er, vs]
            x = (qe * ke).sum(axis=1) * scale
            mass = np.abs(qe * ke).sum(axis=1)
            y = y64[j]
            dy = (ge * ve).sum(axis=1)
            a = (dv + 6) * U * np.abs(ge * ve).sum(axis=1)
            rho, eps_D, ds = np.zeros(E), np.zeros(E), np.zeros(E)
            Lr, segr = np.zeros(E), np.zeros(E)
            for i, L in enumerate(LENS):
                if not L:
                    continue
                lo, hi = int(row_ptr[i]), int(row_ptr[i + 1])
                segs = -(-L // 256)
                t = x[lo:hi] - x[lo:hi].max()
                eta = (abs(scale) * (d + 6) * U * mass[lo:hi] + 3 * U * np.abs(x[lo:hi]) + 2 * U * np.abs(t)).max()
                rho[lo:hi] = (segs + 16 + L + 4) * U + 2 * eta
                T = (y[lo:hi] * np.abs(dy[lo:hi])).sum()
                D = (y[lo:hi] * dy[lo:hi]).sum()
                eps_D[lo:hi] = (L + segs + 12) * U * T + rho[lo] * T + (y[lo:hi] * a[lo:hi]).sum()
                ds[lo:hi] = (dy[lo:hi] - D) * y[lo:hi] * scale
                Lr[lo:hi], segr[lo:hi] = L, segs
            b = (5 * U + rho) * np.abs(ds) + abs(scale) * y * (a + eps_D)
            Lc = col_len[idl].astype(np.float64)
            segc = np.ceil(Lc / 256)
            # dq: per entry the terms of its row; dk, dv: of its column
            bq = np.zeros((nq, d)); bk = np.zeros((N, d)); bv = np.zeros((N, dv))
            np.add.at(bq, er, ((Lr + segr + 2) * U * np.abs(ds) + b)[:, None] * np.abs(ke))
            np.add.at(bk, idl, ((Lc + segc + 2) * U * np.abs(ds) + b)[:, None] * np.abs(qe))
            np.add.at(bv, idl, ((Lc + segc + 2) * U * y + rho * y)[:, None] * np.abs(ge))
            for name, got, ref, bound in (("dq", dq[:, qs], rq[:, qs], bq), ("dk", dk[:, qs], rk[:, qs], bk), ("dv", dvv[:, vs], rv[:, vs], bv)):
                bound = 2 * 1.01 * bound
                err = np.abs(got - ref)
                nz = bound > 0
                assert (err[~nz] == 0).all(), name                    # no entry, no term: both sides are exactly zero
                worst[name] = max(worst[name], float((err[nz] / bound[nz]).max()))
                assert (err <= bound).all(), (name, j, float((err[nz] / bound[nz]).max()))
        print(f"d={d} dv={dv} scale={scale}: worst error / bound = " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_injected_rows_reach_every_boundary():
    rows_fix = abr.injected(2000)
    abr.check_injected(rows_fix)
    import propagate_t_ref as pt
    row_ptr, ids, _ = pt.csr_of(rows_fix)
    st = abr.attention_bwd_stats_ref(row_ptr, ids, 2000)
    assert st["entries"] == 12862 and st["long_rows"] == 2 and st["long_cols"] == 16 and st["max_col"] == 601 and st["columns"] == 2000 - 261
    assert abr.attention_bwd_stats_ref(row_ptr, ids, 2000, 0)["short_cols"] == 0 and abr.attention_bwd_stats_ref(row_ptr, ids, 2000, 1)["short_cols"] == 556


@pytest.fixture(scope="session")
def attn_bwd_plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attn_bwd_plan") / "attn_bwd_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "attn_bwd_plan_check.cpp")], check=True)
    return exe


def test_the_split_of_the_columns_against_brute_force(attn_bwd_plan_check):
    """fora_attn_bwd_plan.h: every non-empty column in exactly one list, every entry covered once, no empty column anywhere, the
    longer columns' plan chunked as PROPAGATE's"""
    rng = np.random.Generator(np.random.PCG64(9940))
    cases = [[0, 1, 255, 256, 257, 600], [1, 0, 255, 0, 0, 256, 257, 0, 600, 0], [], [0, 0], [3, 64, 1, 256, 0, 17],     # (only short columns)
             [257, 600, 1000, 300], [0, 600, 0, 0, 257, 0], [int(x) for x in rng.integers(0, 900, size=40)]]           # (only long columns at 256; empty ones in between)
    for lens in cases:
        for option in (0, 1, 64, 256):
            for per in (1, 2, 3):
                arg = ",".join(map(str, lens)) or "-"
                r = subprocess.run([attn_bwd_plan_check, str(option), str(per), arg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                assert r.returncode == 0 and not r.stderr, (option, per, lens, r.stdout[-500:], r.stderr[-2000:])
                long_cols = sum(1 for L in lens if L > option)
                long_segs = sum(-(-L // 256) for L in lens if L > option)
                chunks = max(1, -(-long_segs // per)) if lens else 0
                assert r.stdout.split() == [f"short={sum(1 for L in lens if 0 < L <= option)}", f"long_cols={long_cols}", f"long_segs={long_segs}",
                                            f"columns={sum(1 for L in lens if L)}", f"chunks={chunks}", "ok"]


def test_abi_surface():
    import inspect
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    assert hdr.index(" * ATTENTION (fora_hip_sparse_attention)") < hdr.index(" * ATTENTION, BACKWARD (fora_hip_sparse_attention_bwd)") < hdr.index(" * PROPAGATE WITH VALUES (")
    # (the fields and sizes of the two structs against the header: tests/test_capi_cpu.py)
    assert capi.STRUCTS["fora_attn_bwd_stats"] is capi.AttnBwdStats and capi.STRUCTS["fora_attn_grads"] is capi.AttnGrads
    product, test = capi.load(), capi.load(capi.TEST_LIB)
    name = "fora_hip_sparse_attention_bwd"
    assert hasattr(product, name) and hasattr(test, name) and name in capi.SYMBOLS
    # NULL ctx: answered without touching the GPU
    fn = product.fora_hip_sparse_attention_bwd
    assert fn(None, None, 0, None, 0, 1, None, 0, 1, None, 0, 1, None, 0, 1, None, 0, 0, 1, 1, 1, 1.0, None, None) == -1
    assert callable(capi.Engine.sparse_attention_bwd)
    sig = inspect.signature(capi.Engine.sparse_attention_bwd)
    assert [sig.parameters[k].default for k in ("heads", "scale", "want_dq", "want_dk", "want_dv", "want32", "want64")] == [1, None, True, True, True, True, False]
    from fora_amd import torch_ops
    assert inspect.signature(torch_ops.ppr_attention_fused).parameters["backward"].default == "calls"
    assert issubclass(torch_ops._PprAttentionFusedBwd, torch_ops._PprAttentionFused)
    with pytest.raises(ValueError):
        torch_ops.ppr_attention_fused(None, None, np.zeros((1, 2)), None, np.zeros((1, 2)), backward="other")
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "sparse_attention_bwd" in open(os.path.join(ROOT, doc)).read(), doc
