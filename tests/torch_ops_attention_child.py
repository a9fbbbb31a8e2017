"""Child process of tests/test_torch_ops_attention_gpu.py: fora_amd.torch_ops.ppr_attention_fused and
ppr_attention(softmax="fused"), forward and backward.  torch is imported first, so that the library binds to the HIP runtime
torch brought along.  The process starts fresh and ends here."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fora_amd  # noqa: E402
from fora_amd import capi, synth  # noqa: E402
from fora_amd.torch_ops import ppr_attention, ppr_attention_fused, row_softmax  # noqa: E402
import attention_ref as ar  # noqa: E402
import propagate_values_ref as pv  # noqa: E402
import sddmm_ref as sr  # noqa: E402
import softmax_ref as sm  # noqa: E402

SEED = 0x464F5241
U32 = 2.0 ** -24


def bits(x):
    a = x.detach().cpu().numpy()
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def main():
    assert torch.cuda.is_available()
    engine = fora_amd.Engine(0, lib=capi.TEST_LIB)          # the build with the row injection
    dev = torch.device("cuda", engine.device)
    n, m, row_ptr_g, col = synth.preset("tiny", "none")
    engine.set_graph(n, m, row_ptr_g, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    row_ptr, _ = engine.test_sparse_rows(sm.injected_rows(n), threshold=0.0)
    nq, e = len(sm.ROW_LENS), int(row_ptr[-1])
    ids = np.zeros(e, np.int32)
    engine.sparse_fetch(ids=ids, cap=e)
    rng = np.random.Generator(np.random.PCG64(9950))
    d, dv, heads, scale = 12, 7, 2, 0.5
    Q0, K0 = ar.scores_operands(rng, nq, n, d, heads)
    V0 = rng.standard_normal((n, heads * dv)).astype(np.float32)
    G0 = rng.standard_normal((nq, heads * dv)).astype(np.float32)
    leaf = lambda x: torch.from_numpy(x).to(dev).requires_grad_(True)
    # ---- forward: the one call; backward: the composition of the existing twins on the saved float32 y, head by head
    for short in (256, 0):
        engine.set_option("attn_short", short)
        Q, K, V = leaf(Q0), leaf(K0), leaf(V0)
        out = ppr_attention_fused(engine, row_ptr, Q, K, V, scale=scale, heads=heads)
        e32, _, _, _, _ = engine.sparse_attention(row_ptr, Q.detach(), K.detach(), V.detach(), heads=heads, scale=scale)
        want64, want32, y64, y32, nan_rows = ar.attention_ref(row_ptr, ids, Q0, K0, V0, d, dv, heads, scale)
        assert nan_rows == 0 and out.dtype == torch.float32 and tuple(out.shape) == (nq, heads * dv)
        assert (bits(out) == bits(e32)).all() and (bits(out) == want32.view(np.uint32)).all()
        out.backward(torch.from_numpy(G0).to(dev))
        for j in range(heads):
            qs, vs = slice(j * d, (j + 1) * d), slice(j * dv, (j + 1) * dv)
            _, want_dv = pv.propagate_t_vals_ref(row_ptr, ids, y32[j], G0[:, vs], n)
            _, dy32 = sr.sddmm_ref(row_ptr, ids, G0[:, vs], V0[:, vs])
            _, ds32 = sm.softmax_bwd_ref(row_ptr, y32[j], dy32, scale)
            _, want_dq = pv.propagate_vals_ref(row_ptr, ids, ds32, K0[:, qs])
            _, want_dk = pv.propagate_t_vals_ref(row_ptr, ids, ds32, Q0[:, qs], n)
            assert (bits(V.grad[:, vs].contiguous()) == want_dv.view(np.uint32)).all(), (short, j)
            assert (bits(Q.grad[:, qs].contiguous()) == want_dq.view(np.uint32)).all() and (bits(K.grad[:, qs].contiguous()) == want_dk.view(np.uint32)).all(), (short, j)
        assert (Q.grad[sm.EMPTY] == 0).all()                  # the empty row attends to nothing
    engine.set_option("attn_short", 256)
    # ---- two heads equal the concatenation of two single-head calls, forward and backward
    G = torch.from_numpy(G0).to(dev)
    singles = []
    for j in range(heads):
        qs, vs = slice(j * d, (j + 1) * d), slice(j * dv, (j + 1) * dv)
        Qj, Kj, Vj = leaf(np.ascontiguousarray(Q0[:, qs])), leaf(np.ascontiguousarray(K0[:, qs])), leaf(np.ascontiguousarray(V0[:, vs]))
        oj = ppr_attention_fused(engine, row_ptr, Qj, Kj, Vj, scale=scale)
        oj.backward(G[:, vs])
        singles.append((oj.detach(), Qj.grad, Kj.grad, Vj.grad))
    cat = [torch.cat([s[i] for s in singles], dim=1) for i in range(4)]
    assert (bits(out) == bits(cat[0])).all() and (bits(Q.grad) == bits(cat[1])).all() and (bits(K.grad) == bits(cat[2])).all() and (bits(V.grad) == bits(cat[3])).all()
    # ---- softmax="fused" routes there with one head; the default scale is d ** -0.5
    Q1, K1, V1 = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (Q0[:, :d], K0[:, :d], V0[:, :dv]))
    out_f = ppr_attention(engine, row_ptr, Q1, K1, V1, softmax="fused")
    assert (bits(out_f) == bits(ppr_attention_fused(engine, row_ptr, Q1, K1, V1))).all()
    assert (bits(out_f) == ar.attention_ref(row_ptr, ids, Q0[:, :d], K0[:, :d], V0[:, :dv], d, dv, 1, float(d) ** -0.5)[1].view(np.uint32)).all()
    # ---- "fused" against "engine".  The engine path rounds twice to float32 where the fused path does not: the scores (the
    # argument of exp moves by at most X 2^-24, X = max |score * scale|, and d log y_e = eps_e - sum_k y_k eps_k turns that into a
    # relative 2 X 2^-24 of y) and y itself (2^-24 of y).  The y of a row sum to 1, so an output moves by at most (2 X + 1) 2^-24
    # max |V|; the outputs are rounded to float32 on either side, 2 * 2^-24 max |V|.  1 % on top for the second order and the
    # float64 arithmetic both share.
    out_e = ppr_attention(engine, row_ptr, Q1, K1, V1, scale=scale, softmax="engine")
    out_f = ppr_attention(engine, row_ptr, Q1, K1, V1, scale=scale, softmax="fused")
    s64, _ = sr.sddmm_ref(row_ptr, ids, Q0[:, :d], K0[:, :d])
    X = float(np.abs(s64 * scale).max())
    tol = 1.01 * (2 * X + 3) * U32 * float(np.abs(V0[:, :dv]).max())
    diff = (out_e.double() - out_f.double()).abs().max().item()
    print(f"ppr_attention engine against fused: max difference {diff:.3e}, bound {tol:.3e}")
    assert diff <= tol
    # ---- the gradients against float64 autograd of the plain expression.  The fused path's backward pass reads y, dy = <G, V>
    # and ds rounded to float32 (2^-24 each) and rounds its three results to float32; everything else is float64 on both sides.
    #   dV[v, c] = sum y_e G[row_e, c]:  2 * 2^-24 sum y_e |G[row_e, c]|   (y's rounding, the result's)
    #   ds_e = (dy_e - D) y_e scale, D = sum y_k dy_k, M = sum y_k |dy_k|:  D moves by 2 * 2^-24 M, dy_e by 2^-24 |dy_e|, the factor
    #     y_e and the result by 2^-24 each on |dy_e - D| <= |dy_e| + M:  E_e = 2^-24 |scale| y_e (3 |dy_e| + 4 M)
    #   dQ[i, c] = sum ds_e K[id_e, c], dK[v, c] = sum ds_e Q[row_e, c]:  sum (E_e + 2^-24 |ds_e|) |K| resp. |Q|
    # 1 % on top for the second order and for autograd's own float64 roundings.
    rows_t = torch.from_numpy(sr.entry_rows(row_ptr)).to(dev)
    ids_t = torch.from_numpy(ids.astype(np.int64)).to(dev)
    Qd, Kd, Vd = (torch.from_numpy(x.astype(np.float64)).to(dev).requires_grad_(True) for x in (Q0[:, :d], K0[:, :d], V0[:, :dv]))
    s_t = (Qd[rows_t] * Kd[ids_t]).sum(dim=1) * scale
    y_t = row_softmax(row_ptr, s_t)
    plain = torch.zeros((nq, dv), dtype=torch.float64, device=dev).index_add(0, rows_t, y_t[:, None] * Vd[ids_t])
    G1 = G[:, :dv].double()
    plain.backward(G1)
    Qf, Kf, Vf = (x.clone().requires_grad_(True) for x in (Q1, K1, V1))
    ppr_attention_fused(engine, row_ptr, Qf, Kf, Vf, scale=scale).backward(G[:, :dv].contiguous())
    with torch.no_grad():
        y = y_t.detach()
        dy = (G1[rows_t] * Vd[ids_t]).sum(dim=1)
        M = torch.zeros(nq, dtype=torch.float64, device=dev).index_add(0, rows_t, y * dy.abs())[rows_t]
        D = torch.zeros(nq, dtype=torch.float64, device=dev).index_add(0, rows_t, y * dy)[rows_t]
        ds = (dy - D) * y * scale
        E = U32 * abs(scale) * y * (3 * dy.abs() + 4 * M) + U32 * ds.abs()
        b_v = 1.01 * 2 * U32 * torch.zeros((n, dv), dtype=torch.float64, device=dev).index_add(0, ids_t, y[:, None] * G1[rows_t].abs())
        b_q = 1.01 * torch.zeros((nq, d), dtype=torch.float64, device=dev).index_add(0, rows_t, E[:, None] * Kd[ids_t].abs())
        b_k = 1.01 * torch.zeros((n, d), dtype=torch.float64, device=dev).index_add(0, ids_t, E[:, None] * Qd[rows_t].abs())
        for name, got, want, bound in (("dV", Vf.grad, Vd.grad, b_v), ("dQ", Qf.grad, Qd.grad, b_q), ("dK", Kf.grad, Kd.grad, b_k)):
            err = (got.double() - want).abs()
            live = bound > 0
            worst = (err[live] / bound[live]).max().item()
            print(f"{name} against float64 autograd: worst error / bound = {worst:.3f}")
            assert (err <= bound).all(), name
    # ---- bfloat16 operands come back with bfloat16 gradients
    Qb, Kb, Vb = (x.to(torch.bfloat16).requires_grad_(True) for x in (Q1, K1, V1))
    ob = ppr_attention_fused(engine, row_ptr, Qb, Kb, Vb, scale=scale)
    ob.backward(G[:, :dv].contiguous())
    assert ob.dtype == torch.float32 and Qb.grad.dtype == Kb.grad.dtype == Vb.grad.dtype == torch.bfloat16
    for bad in (0, 5):
        try:
            ppr_attention_fused(engine, row_ptr, Q1, K1, V1, heads=bad)
        except ValueError:
            pass
        else:
            raise AssertionError("heads that do not divide the columns were accepted")
    # ---- a backward pass after the held rows were replaced raises
    Qg = Q1.clone().requires_grad_(True)
    o = ppr_attention_fused(engine, row_ptr, Qg, K1, V1, scale=scale)
    engine.test_sparse_rows(sm.injected_rows(n), threshold=0.0)          # the same rows again: another held result all the same
    try:
        o.backward(torch.ones_like(o))
    except RuntimeError as err:
        assert "held sparse result" in str(err)
    else:
        raise AssertionError("the backward pass ran over rows that were replaced")
    assert Qg.grad is None
    engine.close()
    print("torch ops attention ok")


if __name__ == "__main__":
    main()
