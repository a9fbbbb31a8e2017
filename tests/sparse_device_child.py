"""Child process of tests/test_sparse_gpu.py::test_device_fetch_and_torch_csr: Engine.query_sparse(device=True) and
capi.to_torch_csr.  torch is imported first, so that the library binds to the HIP runtime torch brought along and a
tensor's data_ptr() is device memory the library knows."""
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
from test_sparse_gpu import SEED, _raw_fetch, check_against_dense, thr_fix_of  # noqa: E402


def main():
    assert torch.cuda.is_available()
    engine = fora_amd.Engine(0)
    for name, dangling in (("tiny", "rmat"), ("small", "none")):
        n, m, row_ptr_g, col = synth.preset(name, dangling)
        deg = np.diff(row_ptr_g)
        rng = np.random.Generator(np.random.PCG64(4400))
        live = rng.choice(np.flatnonzero(deg > 0), 5, replace=False)
        dang = rng.choice(np.flatnonzero(deg == 0), 1) if (deg == 0).any() else np.zeros(0, np.int64)
        srcs = np.concatenate([live[:3], dang, live[3:], live[1:2]]).astype(np.int32)
        engine.set_graph(n, m, row_ptr_g, col)
        engine.set_params(epsilon=0.5, seed=SEED)
        want, _, wst = engine.query_fix(srcs)
        dense_all, _ = engine.query(srcs)
        for t in (None, 1e-3, 0.0):
            thr = thr_fix_of(1.0 / n if t is None else t)
            rp_d, ids_d, vals_d, fix_d, st_d, sp_d = engine.query_sparse(srcs, threshold=t, want_fix=True, device=True)
            for x, dt in ((rp_d, torch.int64), (ids_d, torch.int32), (vals_d, torch.float64), (fix_d, torch.int64)):
                assert x.is_cuda and x.device.index == engine.device and x.dtype == dt
            # the same call's host arrays: the held result, fetched again
            e = sp_d["entries"]
            ids, vals, fix = np.zeros(e, np.int32), np.zeros(e, np.float64), np.zeros(e, np.uint64)
            assert _raw_fetch(engine, ids, vals, fix, e) == 0
            assert (ids_d.cpu().numpy() == ids).all() and (vals_d.cpu().numpy() == vals).all()
            assert (fix_d.cpu().numpy().view(np.uint64) == fix).all()
            check_against_dense(want, wst, thr, rp_d.cpu().numpy(), ids, vals, fix, st_d, sp_d)
            # without fix: five results
            rp2, ids2, vals2, _, _ = engine.query_sparse(srcs, threshold=t, device=True)
            assert torch.equal(rp2, rp_d) and torch.equal(ids2, ids_d) and torch.equal(vals2, vals_d)
            dense = dense_all.copy()
            dense[want < np.uint64(thr)] = 0.0
            csr = capi.to_torch_csr(rp_d, ids_d, vals_d, n)
            assert csr.layout == torch.sparse_csr and tuple(csr.shape) == (len(srcs), n) and csr.is_cuda
            assert (csr.to_dense().cpu().numpy() == dense).all()
    engine.close()
    print("sparse device ok")


if __name__ == "__main__":
    main()
