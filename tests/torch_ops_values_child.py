"""Child process of tests/test_torch_ops_values_gpu.py: fora_amd.torch_ops with the caller's values on the held pattern --
ppr_propagate(values=), ppr_sddmm, ppr_attention -- forward and backward against the numpy twins.  torch is imported first, so
that the library binds to the HIP runtime torch brought along.  The process starts fresh and ends here."""
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
from fora_amd.torch_ops import ppr_attention, ppr_propagate, ppr_sddmm, row_softmax  # noqa: E402
import propagate_ref as pr  # noqa: E402
import propagate_values_ref as pv  # noqa: E402
import sddmm_ref as sr  # noqa: E402

SEED = 0x464F5241


def bits(x):
    a = x.detach().cpu()
    if a.dtype == torch.bfloat16:
        return a.view(torch.int16).numpy()
    return a.numpy().view({4: np.uint32, 8: np.uint64}[a.element_size()])


def host(x):
    """a device tensor as the numpy operand of a twin: (array, bf16?)"""
    a = x.detach().cpu()
    if a.dtype == torch.bfloat16:
        return a.view(torch.int16).numpy().view(np.uint16), True
    return a.numpy(), False


def main():
    assert torch.cuda.is_available()
    engine = fora_amd.Engine(0, lib=capi.TEST_LIB)          # the build with the row injection
    dev = torch.device("cuda", engine.device)
    n, m, row_ptr_g, col = synth.preset("tiny", "none")
    engine.set_graph(n, m, row_ptr_g, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    row_ptr, _ = engine.test_sparse_rows(sr.injected_rows(n), threshold=0.0)
    nq, e = len(sr.ROW_LENS), int(row_ptr[-1])
    ids = np.zeros(e, np.int32)
    engine.sparse_fetch(ids=ids, cap=e)
    rng = np.random.Generator(np.random.PCG64(9900))
    d = 12
    # ---- ppr_propagate(values=): forward, H.grad and values.grad equal the twins' results cast to f32
    for h_dtype in (torch.float32, torch.bfloat16):
        for v_dtype in (torch.float32, torch.float64):
            H0 = torch.from_numpy(pr.scaled_features(rng, n, d)).to(dev).to(h_dtype)
            v0 = torch.from_numpy(pv.distinct_values(rng, e, np.float64)).to(dev).to(v_dtype)
            G = torch.from_numpy(pr.scaled_features(rng, nq, d)).to(dev)
            H, v = H0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
            Z = ppr_propagate(engine, row_ptr, H, values=v)
            (Hh, h_bf16), vh, Gh = host(H0), v0.cpu().numpy(), G.cpu().numpy()
            _, want_z = pv.propagate_vals_ref(row_ptr, ids, vh, Hh, bf16=h_bf16)
            assert Z.dtype == torch.float32 and Z.is_cuda and (bits(Z) == want_z.view(np.uint32)).all(), (h_dtype, v_dtype)
            Z.backward(G)
            _, want_dh = pv.propagate_t_vals_ref(row_ptr, ids, vh, Gh, n)
            _, want_dv = sr.sddmm_ref(row_ptr, ids, Gh, Hh, b_bf16=h_bf16)
            assert H.grad.dtype == h_dtype and tuple(H.grad.shape) == (n, d) and v.grad.dtype == v_dtype and tuple(v.grad.shape) == (e,)
            assert (bits(H.grad) == bits(torch.from_numpy(want_dh).to(h_dtype))).all(), (h_dtype, v_dtype)
            assert (bits(v.grad) == bits(torch.from_numpy(want_dv).to(v_dtype))).all(), (h_dtype, v_dtype)
            # only one of the two wants a gradient
            H, v = H0.clone().requires_grad_(True), v0.clone()
            ppr_propagate(engine, row_ptr, H, values=v).backward(G)
            assert (bits(H.grad) == bits(torch.from_numpy(want_dh).to(h_dtype))).all() and v.grad is None
    # values=None is today's path: the bits of Engine.sparse_propagate, normalised or not
    H0 = torch.from_numpy(pr.scaled_features(rng, n, d)).to(dev)
    for normalize in (False, True):
        z32, _, _ = engine.sparse_propagate(row_ptr, H0, normalize=normalize)
        assert (bits(ppr_propagate(engine, row_ptr, H0, normalize=normalize)) == bits(z32)).all()
    try:
        ppr_propagate(engine, row_ptr, H0, normalize=True, values=torch.ones(e, device=dev))
    except ValueError:
        pass
    else:
        raise AssertionError("normalize together with values was accepted")
    # ---- ppr_sddmm: forward, A.grad and B.grad
    for a_dtype, b_dtype in ((torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16)):
        A0 = torch.from_numpy(pr.scaled_features(rng, nq, d)).to(dev).to(a_dtype)
        B0 = torch.from_numpy(pr.scaled_features(rng, n, d)).to(dev).to(b_dtype)
        g = torch.from_numpy(pv.distinct_values(rng, e, np.float32)).to(dev)
        A, B = A0.clone().requires_grad_(True), B0.clone().requires_grad_(True)
        S = ppr_sddmm(engine, row_ptr, A, B)
        (Ah, a_bf16), (Bh, b_bf16), gh = host(A0), host(B0), g.cpu().numpy()
        _, want_s = sr.sddmm_ref(row_ptr, ids, Ah, Bh, a_bf16=a_bf16, b_bf16=b_bf16)
        assert S.dtype == torch.float32 and S.is_cuda and tuple(S.shape) == (e,) and (bits(S) == want_s.view(np.uint32)).all()
        S.backward(g)
        _, want_da = pv.propagate_vals_ref(row_ptr, ids, gh, Bh, bf16=b_bf16)
        _, want_db = pv.propagate_t_vals_ref(row_ptr, ids, gh, Ah, n, bf16=a_bf16)
        assert A.grad.dtype == a_dtype and tuple(A.grad.shape) == (nq, d) and B.grad.dtype == b_dtype and tuple(B.grad.shape) == (n, d)
        assert (bits(A.grad) == bits(torch.from_numpy(want_da).to(a_dtype))).all(), (a_dtype, b_dtype)
        assert (bits(B.grad) == bits(torch.from_numpy(want_db).to(b_dtype))).all(), (a_dtype, b_dtype)
    # ---- ppr_attention with Q = 0: the softmax of zeros is exactly float32(1 / len), so the output is the values twin's
    lens = np.diff(row_ptr)
    uniform = (np.float32(1.0) / np.repeat(lens, lens).astype(np.float32)).astype(np.float32)
    K = torch.from_numpy(pr.scaled_features(rng, n, d)).to(dev)
    V = torch.from_numpy(pr.scaled_features(rng, n, 7)).to(dev)
    out = ppr_attention(engine, row_ptr, torch.zeros((nq, d), device=dev), K, V)
    _, want = pv.propagate_vals_ref(row_ptr, ids, uniform, V.cpu().numpy())
    assert tuple(out.shape) == (nq, 7) and (bits(out) == want.view(np.uint32)).all()
    # ---- random Q and K: every gradient finite and of the right shape
    Q = torch.from_numpy(rng.standard_normal((nq, d)).astype(np.float32)).to(dev).requires_grad_(True)
    K = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev).requires_grad_(True)
    V = torch.from_numpy(rng.standard_normal((n, 7)).astype(np.float32)).to(dev).requires_grad_(True)
    out = ppr_attention(engine, row_ptr, Q, K, V, scale=0.5)
    out.square().sum().backward()
    for x, shape in ((Q, (nq, d)), (K, (n, d)), (V, (n, 7))):
        assert x.grad is not None and tuple(x.grad.shape) == shape and torch.isfinite(x.grad).all() and x.grad.abs().sum().item() > 0.0
    assert (Q.grad[sr.EMPTY] == 0).all()                      # the empty row attends to nothing
    # the attention rows of the softmax sum to one (a sanity check of row_softmax on the device)
    p = row_softmax(row_ptr, ppr_sddmm(engine, row_ptr, Q.detach(), K.detach()) * 0.5)
    sums = torch.zeros(nq, device=dev).index_add(0, torch.repeat_interleave(torch.arange(nq, device=dev), torch.from_numpy(lens).to(dev)), p)
    assert torch.allclose(sums[torch.from_numpy(lens > 0).to(dev)], torch.ones((), device=dev), atol=1e-5)
    # ---- a backward pass after sparse_clear raises, in every operation
    A = torch.from_numpy(pr.scaled_features(rng, nq, d)).to(dev).requires_grad_(True)
    B = torch.from_numpy(pr.scaled_features(rng, n, d)).to(dev).requires_grad_(True)
    v = torch.ones(e, device=dev, requires_grad=True)
    S = ppr_sddmm(engine, row_ptr, A, B)
    Z = ppr_propagate(engine, row_ptr, B, values=v)
    engine.sparse_clear()
    for y in (S, Z):
        try:
            y.backward(torch.ones_like(y))
        except RuntimeError as err:
            assert "held sparse result" in str(err)
        else:
            raise AssertionError("the backward pass ran over rows that are no longer held")
    assert A.grad is None and B.grad is None and v.grad is None
    engine.close()
    print("torch ops values ok")


if __name__ == "__main__":
    main()
