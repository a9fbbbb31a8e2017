"""Child process of tests/test_propagate_t_gpu.py::test_device_pointers_and_autograd: Engine.sparse_propagate_t with grad and
the outputs in device memory, and fora_amd.torch_ops.ppr_propagate's forward and backward passes.  torch is imported first,
so that the library binds to the HIP runtime torch brought along and a tensor's data_ptr() is device memory the library
knows.  The process starts fresh and ends here."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fora_amd  # noqa: E402
from fora_amd import synth  # noqa: E402
from fora_amd.torch_ops import ppr_propagate  # noqa: E402
import propagate_ref as pr  # noqa: E402
import propagate_t_ref as pt  # noqa: E402

SEED = 0x464F5241


def bits(x):
    a = x.detach().cpu()
    if a.dtype == torch.bfloat16:
        return a.view(torch.int16).numpy()
    return a.numpy().view({4: np.uint32, 8: np.uint64}[a.element_size()])


def main():
    assert torch.cuda.is_available()
    assert "torch" not in open(os.path.join(ROOT, "fora_amd", "__init__.py")).read()
    engine = fora_amd.Engine(0)
    dev = torch.device("cuda", engine.device)
    n, m, row_ptr_g, col = synth.preset("tiny", "rmat")
    deg = np.diff(row_ptr_g)
    rng = np.random.Generator(np.random.PCG64(7900))
    live = rng.choice(np.flatnonzero(deg > 0), 5, replace=False)
    dang = rng.choice(np.flatnonzero(deg == 0), 1)
    srcs = np.concatenate([live[:3], dang, live[3:], live[1:2]]).astype(np.int32)
    nq = len(srcs)
    engine.set_graph(n, m, row_ptr_g, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, threshold=0.0, want_fix=True)
    # ---- device G, contiguous and as a column slice, gives the host path's bits
    for d in (3, 16, 65):
        G = pr.scaled_features(rng, nq, d + 3)
        for normalize in (False, True):
            for bf16 in (False, True):
                if bf16:
                    b16 = pr.to_bf16_bits(G)
                    wide = torch.from_numpy(b16.view(np.int16)).to(dev).view(torch.bfloat16)
                    host_slice, host_cont = b16[:, 1:1 + d], np.ascontiguousarray(b16[:, :d])
                else:
                    wide = torch.from_numpy(G).to(dev)
                    host_slice, host_cont = G[:, 1:1 + d], np.ascontiguousarray(G[:, :d])
                for grad_d, grad_h in ((wide[:, :d].contiguous(), host_cont), (wide[:, 1:1 + d], host_slice)):
                    sliced = grad_h is host_slice
                    assert grad_d.is_cuda and grad_d.stride(0) == (d + 3 if sliced else d)
                    h32, h64, hps = engine.sparse_propagate_t(row_ptr, grad_h, normalize=normalize, bf16=bf16, want64=True)
                    want64, want32 = pt.propagate_t_ref(row_ptr, ids, fix, grad_h, n, normalize=normalize, bf16=bf16)
                    assert (h64.view(np.uint64) == want64.view(np.uint64)).all() and (h32.view(np.uint32) == want32.view(np.uint32)).all()
                    d32, d64, dps = engine.sparse_propagate_t(row_ptr, grad_d, normalize=normalize, want64=True)
                    for x, dt in ((d32, torch.float32), (d64, torch.float64)):
                        assert x.is_cuda and x.device.index == engine.device and x.dtype == dt and tuple(x.shape) == (n, d)
                    assert (bits(d64) == h64.view(np.uint64)).all(), (d, normalize, bf16, sliced)
                    assert (bits(d32) == h32.view(np.uint32)).all(), (d, normalize, bf16, sliced)
                    assert hps["feat_on_device"] == 0 and dps["feat_on_device"] == 1
    # a padded device output keeps its padding; the transposition as device tensors
    Gd = torch.from_numpy(pr.scaled_features(rng, nq, 5)).to(dev)
    pad = torch.full((n, 9), -3.0, dtype=torch.float64, device=dev)
    engine.sparse_propagate_t(row_ptr, Gd, want32=False, out64=pad[:, :5])
    want64, _ = pt.propagate_t_ref(row_ptr, ids, fix, Gd.cpu().numpy(), n)
    got = pad.cpu().numpy()
    assert (got[:, :5].view(np.uint64) == want64.view(np.uint64)).all() and (got[:, 5:] == -3.0).all()
    col_ptr, rows, fix_t = pt.transpose_ref(row_ptr, ids, fix, n)
    c_d, r_d, v_d, f_d = engine.sparse_transpose_fetch(row_ptr, want_fix=True, device=True)
    assert c_d.is_cuda and (c_d.cpu().numpy() == col_ptr).all() and (r_d.cpu().numpy() == rows).all()
    assert (f_d.cpu().numpy().view(np.uint64) == fix_t).all() and (bits(v_d) == pr.weights(fix_t).view(np.uint64)).all()
    # ---- autograd: forward = sparse_propagate, backward = sparse_propagate_t, for f32 and bf16 H
    d = 12
    for normalize in (False, True):
        for dtype in (torch.float32, torch.bfloat16):
            H0 = torch.from_numpy(pr.scaled_features(rng, n, d)).to(dev).to(dtype)
            G = torch.from_numpy(pr.scaled_features(rng, nq, d)).to(dev)
            H = H0.clone().requires_grad_(True)
            Z = ppr_propagate(engine, row_ptr, H, normalize=normalize)
            z32, _, _ = engine.sparse_propagate(row_ptr, H0, normalize=normalize)
            assert Z.dtype == torch.float32 and Z.is_cuda and (bits(Z) == bits(z32)).all()
            Z.backward(G)
            g32, _, _ = engine.sparse_propagate_t(row_ptr, G, normalize=normalize)
            assert H.grad.dtype == dtype and tuple(H.grad.shape) == (n, d)
            assert (bits(H.grad) == bits(g32.to(dtype))).all(), (normalize, dtype)
            if dtype == torch.float32:
                assert (bits(H.grad) == bits(g32)).all()
            # a gradient that is no dense row-major matrix: the sum's expanded ones, a transposed view
            H = H0.clone().requires_grad_(True)
            ppr_propagate(engine, row_ptr, H, normalize=normalize).sum().backward()
            ones32, _, _ = engine.sparse_propagate_t(row_ptr, torch.ones((nq, d), device=dev), normalize=normalize)
            assert (bits(H.grad) == bits(ones32.to(dtype))).all()
            H = H0.clone().requires_grad_(True)
            Gt = G.t().contiguous().t()
            assert Gt.stride(1) != 1
            ppr_propagate(engine, row_ptr, H, normalize=normalize).backward(Gt)
            assert (bits(H.grad) == bits(g32.to(dtype))).all()
    # a backward pass after the held result was replaced raises
    H = torch.from_numpy(pr.scaled_features(rng, n, d)).to(dev).requires_grad_(True)
    Z = ppr_propagate(engine, row_ptr, H)
    engine.query_sparse(srcs[:3], threshold=0.0)
    try:
        Z.backward(torch.ones_like(Z))
    except RuntimeError as err:
        assert "held sparse result" in str(err)
    else:
        raise AssertionError("the backward pass ran over rows that are no longer the forward's")
    assert H.grad is None
    engine.close()
    print("propagate_t device ok")


if __name__ == "__main__":
    main()
