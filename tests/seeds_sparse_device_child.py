"""Child process of tests/test_seeds_sparse_gpu.py::test_device_fetch: Engine.query_seeds_sparse(device=True) and
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
import seeds_outputs_ref as so  # noqa: E402


class G:
    def __init__(self, n, m, row_ptr, col):
        self.n, self.m, self.row_ptr, self.col = n, m, row_ptr, col
        self.deg = np.diff(row_ptr)


def main():
    assert torch.cuda.is_available()
    engine = fora_amd.Engine(0)
    g = G(*synth.preset("tiny", "rmat"))
    so.load(engine, g)
    c = so.reference(engine, g)
    for t in (None, 0.0):
        thr = so.thr_fix_of(1.0 / g.n if t is None else t)
        row_ptr, ids, fix = so.csr_of(c.expect["w"], thr)
        out = engine.query_seeds_sparse(c.sets, weights=c.weights, threshold=t, want_fix=True, device=True)
        for x, dt in ((out["row_ptr"], torch.int64), (out["ids"], torch.int32), (out["vals"], torch.float64), (out["fix"], torch.int64)):
            assert x.is_cuda and x.device.index == engine.device and x.dtype == dt
        assert out["row_ptr"].cpu().tolist() == row_ptr and out["ids"].cpu().tolist() == ids
        assert out["fix"].cpu().numpy().view(np.uint64).tolist() == fix
        vals = np.ldexp(np.array(fix, dtype=np.uint64).astype(np.float64), -62)
        assert np.array_equal(out["vals"].cpu().numpy(), vals)
        assert out["row_sum_fix"].tolist() == [sum(r) for r in c.expect["w"]]
        host = engine.query_seeds_sparse(c.sets, weights=c.weights, threshold=t, want_fix=True)   # the host arrays of the same call
        assert np.array_equal(host["ids"], out["ids"].cpu().numpy()) and np.array_equal(host["vals"], out["vals"].cpu().numpy())
        dense = np.zeros((len(c.sets), g.n))
        for i in range(len(c.sets)):
            lo, hi = row_ptr[i], row_ptr[i + 1]
            dense[i, ids[lo:hi]] = vals[lo:hi]
        csr = capi.to_torch_csr(out["row_ptr"], out["ids"], out["vals"], g.n)
        assert csr.layout == torch.sparse_csr and tuple(csr.shape) == (len(c.sets), g.n) and csr.is_cuda
        assert (csr.to_dense().cpu().numpy() == dense).all()
    engine.close()
    print("seeds sparse device ok")


if __name__ == "__main__":
    main()
