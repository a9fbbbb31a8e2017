"""Child process of tests/test_propagate_gpu.py::test_device_pointers: Engine.sparse_propagate with feat and the outputs
in device memory.  torch is imported first, so that the library binds to the HIP runtime torch brought along and a
tensor's data_ptr() is device memory the library knows.  The process starts fresh and ends here."""
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
import propagate_ref as pr  # noqa: E402

SEED = 0x464F5241


def main():
    assert torch.cuda.is_available()
    # the option "prop_segs" is read from the environment like the other non-schedule knobs, when a context is made
    os.environ["FORA_HIP_PROP_SEGS"] = "3"
    first = fora_amd.Engine(0)
    assert first.get_option("prop_segs") == 3
    first.close()
    del os.environ["FORA_HIP_PROP_SEGS"]
    engine = fora_amd.Engine(0)
    assert engine.get_option("prop_segs") == 0
    dev = torch.device("cuda", engine.device)
    for name, dangling in (("tiny", "rmat"), ("small", "none")):
        n, m, row_ptr_g, col = synth.preset(name, dangling)
        deg = np.diff(row_ptr_g)
        rng = np.random.Generator(np.random.PCG64(6800))
        live = rng.choice(np.flatnonzero(deg > 0), 5, replace=False)
        dang = rng.choice(np.flatnonzero(deg == 0), 1) if (deg == 0).any() else np.zeros(0, np.int64)
        srcs = np.concatenate([live[:3], dang, live[3:], live[1:2]]).astype(np.int32)
        engine.set_graph(n, m, row_ptr_g, col)
        engine.set_params(epsilon=0.5, seed=SEED)
        row_ptr, ids, vals, fix, st, sp = engine.query_sparse(srcs, threshold=0.0 if name == "tiny" else 1.0 / n, want_fix=True)
        assert sp["max_row"] > 256
        for d in (3, 16, 65):
            H = pr.scaled_features(rng, n, d + 3)
            for normalize in (False, True):
                for bf16 in (False, True):
                    if bf16:
                        bits = pr.to_bf16_bits(H)
                        wide = torch.from_numpy(bits.view(np.int16)).to(dev).view(torch.bfloat16)      # [n, d + 3] on the GPU
                        host_slice, host_cont = bits[:, 1:1 + d], np.ascontiguousarray(bits[:, :d])
                    else:
                        wide = torch.from_numpy(H).to(dev)
                        host_slice, host_cont = H[:, 1:1 + d], np.ascontiguousarray(H[:, :d])
                    for feat_d, feat_h in ((wide[:, :d].contiguous(), host_cont), (wide[:, 1:1 + d], host_slice)):
                        sliced = feat_h is host_slice
                        assert feat_d.is_cuda and (feat_d.stride(0) == (d + 3 if sliced else d))
                        # the host-pointer path, held to the twin
                        h32, h64, hps = engine.sparse_propagate(row_ptr, feat_h, normalize=normalize, bf16=bf16, want64=True)
                        want64, want32 = pr.propagate_ref(row_ptr, ids, fix, feat_h, normalize=normalize, bf16=bf16)
                        assert (h64.view(np.uint64) == want64.view(np.uint64)).all() and (h32.view(np.uint32) == want32.view(np.uint32)).all()
                        # the device-pointer path: the same bits, in tensors on the GPU
                        d32, d64, dps = engine.sparse_propagate(row_ptr, feat_d, normalize=normalize, want64=True)
                        for x, dt in ((d32, torch.float32), (d64, torch.float64)):
                            assert x.is_cuda and x.device.index == engine.device and x.dtype == dt and tuple(x.shape) == (len(srcs), d)
                        assert (d64.cpu().numpy().view(np.uint64) == h64.view(np.uint64)).all(), (name, d, normalize, bf16, sliced)
                        assert (d32.cpu().numpy().view(np.uint32) == h32.view(np.uint32)).all(), (name, d, normalize, bf16, sliced)
                        assert hps["feat_on_device"] == 0 and dps["feat_on_device"] == 1
                        assert {k: v for k, v in dps.items() if k.endswith("_ms") is False and k != "feat_on_device"} == \
                               {k: v for k, v in hps.items() if k.endswith("_ms") is False and k != "feat_on_device"}
        # a padded device output keeps its padding; the row_ptr may be the device tensor of query_sparse(device=True)
        rp_d, ids_d, vals_d, _, _ = engine.query_sparse(srcs, threshold=1e-3, device=True)
        feat = torch.from_numpy(pr.scaled_features(rng, n, 5)).to(dev)
        pad = torch.full((len(srcs), 9), -3.0, dtype=torch.float64, device=dev)
        _, o64, _ = engine.sparse_propagate(rp_d, feat, want32=False, out64=pad[:, :5])
        want64, _ = pr.propagate_ref(rp_d.cpu().numpy(), ids_d.cpu().numpy(), engine_fix(engine, int(rp_d[-1])), feat.cpu().numpy())
        got = pad.cpu().numpy()
        assert (got[:, :5].view(np.uint64) == want64.view(np.uint64)).all() and (got[:, 5:] == -3.0).all()
        # the convenience, with a device feat: a device output
        r = engine.propagate(srcs, feat, threshold=1e-3, want64=True, chunk=3)
        assert r["out64"].is_cuda and (r["out64"].cpu().numpy().view(np.uint64) == want64.view(np.uint64)).all()
    engine.close()
    print("propagate device ok")


def engine_fix(engine, e):
    fix = np.zeros(e, np.uint64)
    engine.sparse_fetch(fix=fix, cap=e)
    return fix


if __name__ == "__main__":
    main()
