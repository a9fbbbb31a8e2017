"""Child process of tests/test_torch_ops_attention_bwd_gpu.py: fora_amd.torch_ops.ppr_attention_fused(backward="fused"), the
backward pass as ONE library call.  torch is imported first, so that the library binds to the HIP runtime torch brought along.
The process starts fresh and ends here."""
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
from fora_amd.torch_ops import ppr_attention_fused, row_softmax  # noqa: E402
import attention_bwd_ref as abr  # noqa: E402
import attention_ref as ar  # noqa: E402
import sddmm_ref as sr  # noqa: E402

SEED = 0x464F5241
U32 = 2.0 ** -24


def bits(x):
    a = x.detach().cpu().contiguous().numpy()
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def main():
    assert torch.cuda.is_available()
    engine = fora_amd.Engine(0, lib=capi.TEST_LIB)          # the build with the row injection
    dev = torch.device("cuda", engine.device)
    n, m, row_ptr_g, col = synth.preset("tiny", "none")
    engine.set_graph(n, m, row_ptr_g, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    rows_fix = abr.injected(n)
    row_ptr, _ = engine.test_sparse_rows(rows_fix, threshold=0.0)
    nq, e = rows_fix.shape[0], int(row_ptr[-1])
    ids = np.zeros(e, np.int32)
    engine.sparse_fetch(ids=ids, cap=e)
    empty_rows = np.flatnonzero(np.diff(row_ptr) == 0)
    rng = np.random.Generator(np.random.PCG64(9955))
    d, dv, heads, scale = 12, 7, 2, 0.5
    Q0, K0 = ar.scores_operands(rng, nq, n, d, heads)
    V0 = rng.standard_normal((n, heads * dv)).astype(np.float32)
    G0 = rng.standard_normal((nq, heads * dv)).astype(np.float32)
    leaf = lambda x: torch.from_numpy(x).to(dev).requires_grad_(True)
    G = torch.from_numpy(G0).to(dev)
    # ---- the gradients are Engine.sparse_attention_bwd on the saved float32 y, and the twin's, bit for bit
    for short in (256, 0):
        engine.set_option("attn_short", short)
        Q, K, V = leaf(Q0), leaf(K0), leaf(V0)
        out = ppr_attention_fused(engine, row_ptr, Q, K, V, scale=scale, heads=heads, backward="fused")
        o32, _, y32, _, _ = engine.sparse_attention(row_ptr, Q.detach(), K.detach(), V.detach(), heads=heads, scale=scale, want_y32=True)
        assert (bits(out) == bits(o32)).all()
        out.backward(G)
        dq, _, dk, _, dv_, _, st = engine.sparse_attention_bwd(row_ptr, Q.detach(), K.detach(), V.detach(), G, y32, heads=heads, scale=scale)
        assert (bits(Q.grad) == bits(dq)).all() and (bits(K.grad) == bits(dk)).all() and (bits(V.grad) == bits(dv_)).all(), short
        want = abr.attention_bwd_ref(row_ptr, ids, Q0, K0, V0, G0, y32.cpu().numpy(), n, d, dv, heads, scale)
        for got, w in zip((Q.grad, K.grad, V.grad), want):
            assert got.dtype == torch.float32 and (bits(got) == w.astype(np.float32).view(np.uint32)).all(), short
        assert empty_rows.size and (Q.grad[torch.from_numpy(empty_rows).to(dev)] == 0).all()      # an empty row attends to nothing
    engine.set_option("attn_short", 256)
    # ---- only the gradients autograd asks for are computed
    Qn, Kn, Vn = torch.from_numpy(Q0).to(dev), leaf(K0), torch.from_numpy(V0).to(dev)
    ppr_attention_fused(engine, row_ptr, Qn, Kn, Vn, scale=scale, heads=heads, backward="fused").backward(G)
    assert Qn.grad is None and Vn.grad is None and (bits(Kn.grad) == bits(K.grad)).all()
    # ---- two heads equal the concatenation of two single-head calls
    singles = []
    for j in range(heads):
        qs, vs = slice(j * d, (j + 1) * d), slice(j * dv, (j + 1) * dv)
        Qj, Kj, Vj = leaf(np.ascontiguousarray(Q0[:, qs])), leaf(np.ascontiguousarray(K0[:, qs])), leaf(np.ascontiguousarray(V0[:, vs]))
        oj = ppr_attention_fused(engine, row_ptr, Qj, Kj, Vj, scale=scale, backward="fused")
        oj.backward(G[:, vs])                                 # (a column slice: read in place)
        singles.append((oj.detach(), Qj.grad, Kj.grad, Vj.grad))
    cat = [torch.cat([s[i] for s in singles], dim=1) for i in range(4)]
    assert (bits(out) == bits(cat[0])).all() and (bits(Q.grad) == bits(cat[1])).all() and (bits(K.grad) == bits(cat[2])).all() and (bits(V.grad) == bits(cat[3])).all()
    # ---- the gradients against float64 autograd of the plain expression, inside the bounds tests/torch_ops_attention_child.py
    # derives for the head-by-head path, taken unchanged.  The one call makes a strict subset of that path's roundings -- y32 and the
    # final float32, but neither dy nor ds -- so those bounds hold for it.
    #   dV[v, c] = sum y_e G[row_e, c]:  2 * 2^-24 sum y_e |G[row_e, c]|   (y's rounding, the result's)
    #   ds_e = (dy_e - D) y_e scale, D = sum y_k dy_k, M = sum y_k |dy_k|:  E_e = 2^-24 |scale| y_e (3 |dy_e| + 4 M)
    #   dQ[i, c] = sum ds_e K[id_e, c], dK[v, c] = sum ds_e Q[row_e, c]:  sum (E_e + 2^-24 |ds_e|) |K| resp. |Q|
    # 1 % on top for the second order and for autograd's own float64 roundings.
    Q1, K1, V1 = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (Q0[:, :d], K0[:, :d], V0[:, :dv]))
    rows_t = torch.from_numpy(sr.entry_rows(row_ptr)).to(dev)
    ids_t = torch.from_numpy(ids.astype(np.int64)).to(dev)
    Qd, Kd, Vd = (torch.from_numpy(x.astype(np.float64)).to(dev).requires_grad_(True) for x in (Q0[:, :d], K0[:, :d], V0[:, :dv]))
    s_t = (Qd[rows_t] * Kd[ids_t]).sum(dim=1) * scale
    y_t = row_softmax(row_ptr, s_t)
    plain = torch.zeros((nq, dv), dtype=torch.float64, device=dev).index_add(0, rows_t, y_t[:, None] * Vd[ids_t])
    G1 = G[:, :dv].double()
    plain.backward(G1)
    Qf, Kf, Vf = (x.clone().requires_grad_(True) for x in (Q1, K1, V1))
    ppr_attention_fused(engine, row_ptr, Qf, Kf, Vf, scale=scale, backward="fused").backward(G[:, :dv].contiguous())
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
        for name, got, want_g, bound in (("dV", Vf.grad, Vd.grad, b_v), ("dQ", Qf.grad, Qd.grad, b_q), ("dK", Kf.grad, Kd.grad, b_k)):
            err = (got.double() - want_g).abs()
            live = bound > 0
            worst = (err[live] / bound[live]).max().item()
            print(f"{name} (backward=\"fused\") against float64 autograd: worst error / bound = {worst:.3f}")
            assert (err <= bound).all(), name
    # ---- bfloat16 operands come back with bfloat16 gradients
    Qb, Kb, Vb = (x.to(torch.bfloat16).requires_grad_(True) for x in (Q1, K1, V1))
    ob = ppr_attention_fused(engine, row_ptr, Qb, Kb, Vb, scale=scale, backward="fused")
    ob.backward(G[:, :dv].contiguous().to(torch.bfloat16))
    assert ob.dtype == torch.float32 and Qb.grad.dtype == Kb.grad.dtype == Vb.grad.dtype == torch.bfloat16
    assert tuple(Qb.grad.shape) == (nq, d) and tuple(Kb.grad.shape) == (n, d) and tuple(Vb.grad.shape) == (n, dv)
    try:
        ppr_attention_fused(engine, row_ptr, Q1, K1, V1, backward="both")
    except ValueError:
        pass
    else:
        raise AssertionError('backward="both" was accepted')
    # ---- a backward pass after the held rows were replaced raises
    Qg = Q1.clone().requires_grad_(True)
    o = ppr_attention_fused(engine, row_ptr, Qg, K1, V1, scale=scale, backward="fused")
    engine.test_sparse_rows(rows_fix, threshold=0.0)          # the same rows again: another held result all the same
    try:
        o.backward(torch.ones_like(o))
    except RuntimeError as err:
        assert "held sparse result" in str(err)
    else:
        raise AssertionError("the backward pass ran over rows that were replaced")
    assert Qg.grad is None
    engine.close()
    print("torch ops attention bwd ok")


if __name__ == "__main__":
    main()
