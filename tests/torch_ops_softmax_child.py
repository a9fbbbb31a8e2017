"""Child process of tests/test_torch_ops_softmax_gpu.py: fora_amd.torch_ops.ppr_row_softmax and ppr_attention(softmax="engine"),
forward and backward against the numpy twins.  torch is imported first, so that the library binds to the HIP runtime torch
brought along.  The process starts fresh and ends here."""
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
from fora_amd.torch_ops import ppr_attention, ppr_row_softmax  # noqa: E402
import propagate_values_ref as pv  # noqa: E402
import sddmm_ref as sr  # noqa: E402
import softmax_ref as sm  # noqa: E402

SEED = 0x464F5241


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
    rng = np.random.Generator(np.random.PCG64(9600))
    # ---- ppr_row_softmax: the forward output and the gradient equal the twins' f32 results, the gradient in the scores' dtype
    for s_dtype in (np.float32, np.float64):
        for scale in (1.0, 0.37, -2.0):
            s_h = ((rng.random(e) * 2 - 1) * 30).astype(s_dtype)
            g_h = rng.standard_normal(e).astype(np.float32)
            s = torch.from_numpy(s_h).to(dev).requires_grad_(True)
            y = ppr_row_softmax(engine, row_ptr, s, scale)
            _, want_y, _ = sm.softmax_ref(row_ptr, s_h, scale)
            assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == (e,) and (bits(y) == want_y.view(np.uint32)).all(), (s_dtype, scale)
            y.backward(torch.from_numpy(g_h).to(dev))
            _, want_dx = sm.softmax_bwd_ref(row_ptr, want_y, g_h, scale)
            assert s.grad.dtype == s.dtype and tuple(s.grad.shape) == (e,)
            assert (bits(s.grad) == want_dx.astype(s_dtype).view({4: np.uint32, 8: np.uint64}[np.dtype(s_dtype).itemsize])).all(), (s_dtype, scale)
    # ---- ppr_attention(softmax="engine"): the composition of the three twins, forward and backward
    d, dv, scale = 12, 7, 0.5
    Q0 = rng.standard_normal((nq, d)).astype(np.float32)
    K0 = rng.standard_normal((n, d)).astype(np.float32)
    V0 = rng.standard_normal((n, dv)).astype(np.float32)
    G0 = rng.standard_normal((nq, dv)).astype(np.float32)
    Q, K, V = (torch.from_numpy(x).to(dev).requires_grad_(True) for x in (Q0, K0, V0))
    out = ppr_attention(engine, row_ptr, Q, K, V, scale=scale, softmax="engine")
    _, s32 = sr.sddmm_ref(row_ptr, ids, Q0, K0)
    _, y32, nan_rows = sm.softmax_ref(row_ptr, s32, scale)
    _, want = pv.propagate_vals_ref(row_ptr, ids, y32, V0)
    assert nan_rows == 0 and tuple(out.shape) == (nq, dv) and (bits(out) == want.view(np.uint32)).all()
    out.backward(torch.from_numpy(G0).to(dev))
    _, want_dv = pv.propagate_t_vals_ref(row_ptr, ids, y32, G0, n)
    _, dy32 = sr.sddmm_ref(row_ptr, ids, G0, V0)
    _, ds32 = sm.softmax_bwd_ref(row_ptr, y32, dy32, scale)
    _, want_dq = pv.propagate_vals_ref(row_ptr, ids, ds32, K0)
    _, want_dk = pv.propagate_t_vals_ref(row_ptr, ids, ds32, Q0, n)
    assert (bits(V.grad) == want_dv.view(np.uint32)).all()
    assert (bits(Q.grad) == want_dq.view(np.uint32)).all() and (bits(K.grad) == want_dk.view(np.uint32)).all()
    assert (Q.grad[sm.EMPTY] == 0).all()                      # the empty row attends to nothing
    # the default scale is d ** -0.5, folded into the call
    out_d = ppr_attention(engine, row_ptr, Q.detach(), K.detach(), V.detach(), softmax="engine")
    _, y_d, _ = sm.softmax_ref(row_ptr, s32, float(d) ** -0.5)
    assert (bits(out_d) == pv.propagate_vals_ref(row_ptr, ids, y_d, V0)[1].view(np.uint32)).all()
    # ---- the two softmax settings agree.  Both read the same f32 scores s.  The torch path rounds x = s * scale and x - m to
    # f32, an absolute error of at most (|x| + |x - m|) 2^-24 <= 3 X 2^-24 in exp's argument (X = max |x|), which exp turns into a
    # relative one; its f32 exp and division add a few ulp, its row sum of L positive terms in some order at most (L - 1) 2^-24.
    # The engine's y is the f64 result rounded once: 2^-24.  So |y_torch - y_engine| <= (3 X + L + 8) 2^-24 y, and since the y
    # of a row sum to 1 an output differs by at most that factor times max |V|, plus the two f32 roundings of the outputs
    # themselves, 2 * 2^-24 max |V|: (3 X + L + 10) 2^-24 max |V|.
    out_t = ppr_attention(engine, row_ptr, Q.detach(), K.detach(), V.detach(), scale=scale)
    out_e = ppr_attention(engine, row_ptr, Q.detach(), K.detach(), V.detach(), scale=scale, softmax="engine")
    X, L = float(np.abs(s32.astype(np.float64) * scale).max()), int(np.diff(row_ptr).max())
    tol = (3 * X + L + 10) * 2.0 ** -24 * float(np.abs(V0).max())
    diff = (out_t.double() - out_e.double()).abs().max().item()
    print(f"ppr_attention torch against engine softmax: max difference {diff:.3e}, bound {tol:.3e}")
    assert diff <= tol
    try:
        ppr_attention(engine, row_ptr, Q.detach(), K.detach(), V.detach(), softmax="other")
    except ValueError:
        pass
    else:
        raise AssertionError("an unknown softmax setting was accepted")
    # ---- a backward pass after sparse_clear raises
    s = torch.zeros(e, device=dev, requires_grad=True)
    y = ppr_row_softmax(engine, row_ptr, s)
    engine.sparse_clear()
    try:
        y.backward(torch.ones_like(y))
    except RuntimeError as err:
        assert "held sparse result" in str(err)
    else:
        raise AssertionError("the backward pass ran over rows that are no longer held")
    assert s.grad is None
    engine.close()
    print("torch ops softmax ok")


if __name__ == "__main__":
    main()
