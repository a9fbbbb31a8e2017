"""Child process of tests/test_sparse_topk_gpu.py::test_device_fetch_and_autograd: Engine.query_sparse_topk(device=True) and
one forward and backward pass of fora_amd.torch_ops.ppr_propagate over the held top-k rows.  torch is imported first, so that
the library binds to the HIP runtime torch brought along and a tensor's data_ptr() is device memory the library knows.  The
process starts fresh and ends here."""
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
from fora_amd.torch_ops import ppr_propagate  # noqa: E402
import propagate_ref as pr  # noqa: E402
import propagate_t_ref as pt  # noqa: E402
from sparse_topk_ref import check_topk  # noqa: E402

SEED = 0x464F5241


def main():
    assert torch.cuda.is_available()
    engine = fora_amd.Engine(0)
    dev = torch.device("cuda", engine.device)
    n, m, row_ptr_g, col = synth.preset("tiny", "rmat")
    deg = np.diff(row_ptr_g)
    rng = np.random.Generator(np.random.PCG64(9300))
    live = rng.choice(np.flatnonzero(deg > 0), 5, replace=False)
    dang = rng.choice(np.flatnonzero(deg == 0), 1)
    srcs = np.concatenate([live[:3], dang, live[3:], live[1:2]]).astype(np.int32)
    nq, k = len(srcs), 7
    engine.set_graph(n, m, row_ptr_g, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    want, _, _ = engine.query_fix(srcs)
    rp_d, ids_d, vals_d, fix_d, st, sp, tk = engine.query_sparse_topk(srcs, k, threshold=0.0, want_fix=True, device=True)
    for x, dt in ((rp_d, torch.int64), (ids_d, torch.int32), (vals_d, torch.float64), (fix_d, torch.int64)):
        assert x.is_cuda and x.device.index == engine.device and x.dtype == dt
    row_ptr, ids, fix = rp_d.cpu().numpy(), ids_d.cpu().numpy(), fix_d.cpu().numpy().view(np.uint64)
    check_topk(want, 1, k, row_ptr, ids, fix, sp, tk, live=deg[srcs] > 0)
    assert tk["cut_rows"] == 6 and (vals_d.cpu().numpy() == np.ldexp(fix.astype(np.float64), -62)).all()
    csr = capi.to_torch_csr(rp_d, ids_d, vals_d, n)
    assert csr.layout == torch.sparse_csr and tuple(csr.shape) == (nq, n) and csr.is_cuda
    # one forward and one backward pass over the top-k rows
    d = 12
    H0 = torch.from_numpy(pr.scaled_features(rng, n, d)).to(dev)
    G = torch.from_numpy(pr.scaled_features(rng, nq, d)).to(dev)
    for normalize in (False, True):
        H = H0.clone().requires_grad_(True)
        Z = ppr_propagate(engine, row_ptr, H, normalize=normalize)
        _, z32 = pr.propagate_ref(row_ptr, ids, fix, H0.cpu().numpy(), normalize=normalize)
        assert Z.is_cuda and (Z.detach().cpu().numpy().view(np.uint32) == z32.view(np.uint32)).all()
        Z.backward(G)
        _, g32 = pt.propagate_t_ref(row_ptr, ids, fix, G.cpu().numpy(), n, normalize=normalize)
        assert (H.grad.cpu().numpy().view(np.uint32) == g32.view(np.uint32)).all()
    engine.close()
    print("sparse topk device ok")


if __name__ == "__main__":
    main()
