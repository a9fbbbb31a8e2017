"""Child process of tests/test_softmax_gpu.py::test_device_operands_and_outputs: Engine.sparse_softmax and
Engine.sparse_softmax_bwd with the inputs and the outputs in device memory.  torch is imported first, so that the library
binds to the HIP runtime torch brought along and a tensor's data_ptr() is device memory the library knows.  The process
starts fresh and ends here."""
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
    e = int(row_ptr[-1])
    rng = np.random.Generator(np.random.PCG64(9500))
    for dtype in (np.float32, np.float64):
        s_h = ((rng.random(e) * 2 - 1) * 30).astype(dtype)
        g_h = rng.standard_normal(e).astype(dtype)
        s_d, g_d = torch.from_numpy(s_h).to(dev), torch.from_numpy(g_h).to(dev)
        for short in (256, 0):
            engine.set_option("softmax_short", short)
            want64, want32, _ = sm.softmax_ref(row_ptr, s_h, 0.37)
            h32, h64, hst = engine.sparse_softmax(row_ptr, s_h, scale=0.37, want64=True)
            d32, d64, dst = engine.sparse_softmax(row_ptr, s_d, scale=0.37, want64=True)
            for x, dt in ((d32, torch.float32), (d64, torch.float64)):
                assert x.is_cuda and x.device.index == engine.device and x.dtype == dt and tuple(x.shape) == (e,)
            assert (h64.view(np.uint64) == want64.view(np.uint64)).all() and (h32.view(np.uint32) == want32.view(np.uint32)).all()
            assert (bits(d64) == want64.view(np.uint64)).all() and (bits(d32) == want32.view(np.uint32)).all(), (dtype, short)
            assert hst["in_on_device"] == 0 and dst["in_on_device"] == 1 and dst["grad_on_device"] == 0
            # a device input and host outputs, longer than the entries; a host input and a device output
            o32, o64 = np.full(e + 2, -3.0, np.float32), np.full(e + 2, -3.0, np.float64)
            engine.sparse_softmax(row_ptr, s_d, scale=0.37, out32=o32, out64=o64)
            assert (o64[:e].view(np.uint64) == want64.view(np.uint64)).all() and (o32[:e].view(np.uint32) == want32.view(np.uint32)).all()
            assert (o32[e:] == -3.0).all() and (o64[e:] == -3.0).all()
            t64 = torch.full((e + 2,), -3.0, dtype=torch.float64, device=dev)
            engine.sparse_softmax(row_ptr, s_h, scale=0.37, want32=False, out64=t64)
            assert (bits(t64[:e]) == want64.view(np.uint64)).all() and (t64[e:] == -3.0).all()
            # the backward call: y as the f32 output on the device, grad on the device or on the host
            b64, b32 = sm.softmax_bwd_ref(row_ptr, want32, g_h, 0.37)
            x32, x64, xst = engine.sparse_softmax_bwd(row_ptr, d32, g_d, scale=0.37, want64=True)
            assert x64.is_cuda and (bits(x64) == b64.view(np.uint64)).all() and (bits(x32) == b32.view(np.uint32)).all(), (dtype, short)
            assert xst["in_on_device"] == 1 and xst["grad_on_device"] == 1
            m32, m64, mst = engine.sparse_softmax_bwd(row_ptr, d32, g_h, scale=0.37, want64=True)
            assert m64.is_cuda and (bits(m64) == b64.view(np.uint64)).all() and mst["in_on_device"] == 1 and mst["grad_on_device"] == 0
            # a strided tensor is made contiguous by the binding
            wide = torch.stack([s_d, s_d + 1], dim=1)
            v32, _, _ = engine.sparse_softmax(row_ptr, wide[:, 0], scale=0.37)
            assert (bits(v32) == want32.view(np.uint32)).all()
    engine.close()
    print("softmax device ok")


if __name__ == "__main__":
    main()
