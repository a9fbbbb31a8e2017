"""Child process of tests/test_sddmm_gpu.py::test_device_operands_and_outputs: Engine.sparse_sddmm with a, b and the outputs in
device memory.  torch is imported first, so that the library binds to the HIP runtime torch brought along and a tensor's
data_ptr() is device memory the library knows.  The process starts fresh and ends here."""
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
import propagate_ref as pr  # noqa: E402
import sddmm_ref as sr  # noqa: E402

SEED = 0x464F5241


def bits(x):
    a = x.detach().cpu().numpy()
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def on_device(host, bf16, dev):
    """a numpy operand (float32, or uint16 bf16 patterns) as a device tensor of the same bits"""
    if bf16:
        return torch.from_numpy(np.ascontiguousarray(host).view(np.int16)).to(dev).view(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(host)).to(dev)


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
    rng = np.random.Generator(np.random.PCG64(9100))
    for d in (3, 64, 130):
        A32, B32 = pr.scaled_features(rng, nq, d), pr.scaled_features(rng, n, d + 4)
        for a_bf16 in (False, True):
            for b_bf16 in (False, True):
                A = pr.to_bf16_bits(A32) if a_bf16 else A32
                Bw = pr.to_bf16_bits(B32) if b_bf16 else B32
                A_d, Bw_d = on_device(A, a_bf16, dev), on_device(Bw, b_bf16, dev)
                for off in (0, 1, 3):                           # b: the first d columns made contiguous, and slices at odd offsets
                    B_h = np.ascontiguousarray(Bw[:, :d]) if off == 0 else Bw[:, off:off + d]
                    B_d = Bw_d[:, :d].contiguous() if off == 0 else Bw_d[:, off:off + d]
                    assert B_d.stride(0) == (d if off == 0 else d + 4) and B_d.storage_offset() == off
                    what = (d, a_bf16, b_bf16, off)
                    want64, want32 = sr.sddmm_ref(row_ptr, ids, A, B_h, a_bf16=a_bf16, b_bf16=b_bf16)
                    h32, h64, hst = engine.sparse_sddmm(row_ptr, A, B_h, want64=True, a_bf16=a_bf16, b_bf16=b_bf16)
                    assert (h64.view(np.uint64) == want64.view(np.uint64)).all() and (h32.view(np.uint32) == want32.view(np.uint32)).all(), what
                    d32, d64, dst = engine.sparse_sddmm(row_ptr, A_d, B_d, want64=True)
                    for x, dt in ((d32, torch.float32), (d64, torch.float64)):
                        assert x.is_cuda and x.device.index == engine.device and x.dtype == dt and tuple(x.shape) == (e,)
                    assert (bits(d64) == want64.view(np.uint64)).all() and (bits(d32) == want32.view(np.uint32)).all(), what
                    assert hst["a_on_device"] == 0 and hst["b_on_device"] == 0 and dst["a_on_device"] == 1 and dst["b_on_device"] == 1
                # a on the host and b on the device; device operands and host outputs
                m32, m64, mst = engine.sparse_sddmm(row_ptr, A, Bw_d[:, 1:1 + d], want64=True, a_bf16=a_bf16)
                want64, want32 = sr.sddmm_ref(row_ptr, ids, A, Bw[:, 1:1 + d], a_bf16=a_bf16, b_bf16=b_bf16)
                assert m64.is_cuda and (bits(m64) == want64.view(np.uint64)).all() and (bits(m32) == want32.view(np.uint32)).all()
                assert mst["a_on_device"] == 0 and mst["b_on_device"] == 1
                o32, o64 = np.full(e + 2, -3.0, np.float32), np.full(e + 2, -3.0, np.float64)
                engine.sparse_sddmm(row_ptr, A_d, Bw_d[:, 1:1 + d], out32=o32, out64=o64)
                assert (o64[:e].view(np.uint64) == want64.view(np.uint64)).all() and (o32[:e].view(np.uint32) == want32.view(np.uint32)).all()
                assert (o32[e:] == -3.0).all() and (o64[e:] == -3.0).all()
    engine.close()
    print("sddmm device ok")


if __name__ == "__main__":
    main()
