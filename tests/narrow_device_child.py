"""Child process of tests/test_narrow_gpu.py::test_alignment_device_memory_and_autograd: NARROW OPERANDS as torch tensors on the
GPU -- float16, float8_e4m3fn and float8_e5m2, contiguous and as column slices of a wider tensor at an odd and at an even pitch,
read in place -- and the torch_ops functions with float16 leaves and FP8 constants.  torch is imported first, so that the library
binds to the HIP runtime torch brought along and a tensor's data_ptr() is device memory the library knows."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import narrow_ref as nr  # noqa: E402
import fora_amd  # noqa: E402
from fora_amd import synth, torch_ops  # noqa: E402
from test_sparse_gpu import SEED  # noqa: E402

DTYPE = {nr.F16: torch.float16, nr.E4M3: torch.float8_e4m3fn, nr.E5M2: torch.float8_e5m2}


def same(a, b, name):
    """equal bits; NaN compared in NaN-ness (there is none here, but the rule is the suite's)"""
    assert a.shape == b.shape and a.dtype == b.dtype, name
    nan = torch.isnan(b)
    assert torch.equal(torch.isnan(a), nan), name
    view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    assert torch.equal(a.contiguous().view(view)[~nan], b.contiguous().view(view)[~nan]), name


def main():
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    engine = fora_amd.Engine(0)
    n, m, row_ptr_g, col = synth.preset("tiny", "none")
    assert n == 2000
    engine.set_graph(n, m, row_ptr_g, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    rng = np.random.Generator(np.random.PCG64(9750))
    lens = [0, 1, 65, 300, 17]
    rows = [np.sort(rng.choice(n, size=L, replace=False)) for L in lens]
    store_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate(rows).astype(np.int32)
    engine.store_load(store_ptr, ids, rng.integers(1, 1 << 50, size=ids.size, dtype=np.uint64))
    row_ptr, _ = engine.store_take(np.arange(len(lens)))
    nq, e = len(lens), int(row_ptr[-1])

    def tensors(kind, shape):
        """(the codes as a tensor of the type, their widening as a float32 tensor), both on the device"""
        codes = nr.moderate_codes(rng, kind, shape)
        t = torch.from_numpy(codes.view(np.int16) if kind == nr.F16 else codes).to(dev).view(DTYPE[kind])
        return t, torch.from_numpy(nr.widen(kind, codes)).to(dev)

    # ---- alignment: contiguous, and column slices at an odd and an even pitch; (4, 21) is an aligned slice whose last lane
    # reads a tail
    d = 40
    A32 = torch.from_numpy(rng.standard_normal((nq, d)).astype(np.float32)).to(dev)
    for kind in (nr.F16, nr.E4M3, nr.E5M2):
        size = DTYPE[kind].itemsize
        for pitch in (45, 48):
            W, W32 = tensors(kind, (n, pitch))
            for c0, w in ((0, pitch), (1, d), (3, d), (4, 21)):
                X, X32 = W[:, c0:c0 + w], W32[:, c0:c0 + w].contiguous()
                assert X.data_ptr() == W.data_ptr() + c0 * size and (w == pitch) == X.is_contiguous()
                name = f"{kind} pitch {pitch} columns {c0}..{c0 + w}"
                for norm in (False, True):
                    g32, g64, st = engine.sparse_propagate(row_ptr, X, normalize=norm, want32=True, want64=True)
                    w32, w64, _ = engine.sparse_propagate(row_ptr, X32, normalize=norm, want32=True, want64=True)
                    same(g32, w32, name + " propagate 32")
                    same(g64, w64, name + " propagate 64")
                    assert st["feat_bytes"] == e * w * size and st["feat_on_device"] == 1
                assert float(w64.abs().sum()) > 0
                if w == d:
                    g32, g64, st = engine.sparse_sddmm(row_ptr, A32, X, want32=True, want64=True)
                    w32, w64, _ = engine.sparse_sddmm(row_ptr, A32, X32, want32=True, want64=True)
                    same(g32, w32, name + " sddmm 32")
                    same(g64, w64, name + " sddmm 64")
                    assert st["bytes"] == e * d * (4 + size) and st["b_on_device"] == 1
        # the transposed product reads a narrow gradient
        G, G32 = tensors(kind, (nq, 24))
        g32, _, st = engine.sparse_propagate_t(row_ptr, G[:, 1:22], want32=True)
        w32, _, _ = engine.sparse_propagate_t(row_ptr, G32[:, 1:22].contiguous(), want32=True)
        same(g32, w32, f"{kind} propagate_t")
        assert st["feat_bytes"] == e * 21 * size

    # ---- torch_ops with float16 leaves: the gradients come back in float16, equal to the float32 run's rounded to float16
    heads, dq, dv = 2, 8, 6
    H16, H32 = tensors(nr.F16, (n, 12))
    A16, A32 = tensors(nr.F16, (nq, 12))
    B16, B32 = tensors(nr.F16, (n, 12))
    Q16, Q32 = tensors(nr.F16, (nq, heads * dq))
    K16, K32 = tensors(nr.F16, (n, heads * dq))
    V16, V32 = tensors(nr.F16, (n, heads * dv))
    Wz = torch.from_numpy(rng.standard_normal((nq, 12)).astype(np.float32)).to(dev)
    Ws = torch.from_numpy(rng.standard_normal(e).astype(np.float32)).to(dev)
    Wo = torch.from_numpy(rng.standard_normal((nq, heads * dv)).astype(np.float32)).to(dev)

    def run(fn, weight, *leaves):
        xs = [x.clone().requires_grad_(True) for x in leaves]
        out = fn(*xs)
        assert out.dtype == torch.float32
        (out * weight).sum().backward()
        return [out.detach()] + [x.grad for x in xs]

    cases = (("ppr_propagate", lambda H: torch_ops.ppr_propagate(engine, row_ptr, H), Wz, (H16,), (H32,)),
             ("ppr_sddmm", lambda A, B: torch_ops.ppr_sddmm(engine, row_ptr, A, B), Ws, (A16, B16), (A32, B32)),
             ("ppr_attention_fused", lambda Q, K, V: torch_ops.ppr_attention_fused(engine, row_ptr, Q, K, V, heads=heads, backward="fused"), Wo,
              (Q16, K16, V16), (Q32, K32, V32)))
    for name, fn, weight, narrow, wide in cases:
        got, want = run(fn, weight, *narrow), run(fn, weight, *wide)
        same(got[0], want[0], name + " forward")
        for g, w in zip(got[1:], want[1:]):
            assert g.dtype == torch.float16 and w.dtype == torch.float32 and float(w.abs().sum()) > 0, name
            same(g, w.to(torch.float16), name + " gradient")

    # ---- FP8 K and V are constants: the forward pass runs and Q gets its gradient; one that requires grad is refused
    for kind in (nr.E4M3, nr.E5M2):
        K8, K32 = tensors(kind, (n, heads * dq))
        V8, V32 = tensors(kind, (n, heads * dv))
        for backward in ("fused", "calls"):
            outs = []
            for K, V in ((K8, V8), (K32, V32)):
                Q = Q32.clone().requires_grad_(True)
                out = torch_ops.ppr_attention_fused(engine, row_ptr, Q, K, V, heads=heads, backward=backward)
                (out * Wo).sum().backward()
                outs.append((out.detach(), Q.grad))
            same(outs[0][0], outs[1][0], f"{kind} constants forward")
            same(outs[0][1], outs[1][1], f"{kind} constants dQ")
            assert float(outs[1][1].abs().sum()) > 0
        gen = engine.get_option("sparse_generation")
        K8g = K8.clone().requires_grad_(True)
        for call in (lambda: torch_ops.ppr_attention_fused(engine, row_ptr, Q32, K8g, V8, heads=heads),
                     lambda: torch_ops.ppr_attention(engine, row_ptr, Q32[:, :dq], K8g[:, :dq], V8[:, :dv], softmax="engine"),
                     lambda: torch_ops.ppr_sddmm(engine, row_ptr, Q32, K8g),
                     lambda: torch_ops.ppr_propagate(engine, row_ptr, K8g)):
            try:
                call()
                raise AssertionError("an FP8 tensor that requires grad was accepted")
            except ValueError as err:
                assert "FP8" in str(err)
        assert engine.get_option("sparse_generation") == gen
    engine.close()
    print("narrow device ok")


if __name__ == "__main__":
    main()
