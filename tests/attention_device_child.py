"""Child process of tests/test_attention_gpu.py::test_device_operands_and_outputs: Engine.sparse_attention with the operands and
the outputs in device memory.  torch is imported first, so that the library binds to the HIP runtime torch brought along and a
tensor's data_ptr() is device memory the library knows.  The process starts fresh and ends here."""
import ctypes as C
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
import attention_ref as ar  # noqa: E402
import propagate_ref as pr  # noqa: E402
import softmax_ref as sm  # noqa: E402

SEED = 0x464F5241


def bits(x):
    a = x.detach().cpu().numpy()
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr() if torch.is_tensor(x) else x.ctypes.data)


def raw_attention(engine, rp, nq, q, k, v, d, dv, heads, o32, o64, ldo, y64, ycap):
    """fora_hip_sparse_attention itself, every pointer as given (f32 operands, rows back to back); the stats"""
    st = capi.AttnStats()
    engine._chk(engine._lib.fora_hip_sparse_attention(engine._ctx, ptr(rp), C.c_int(nq), ptr(q), C.c_int(capi.PROP_F32), C.c_int64(heads * d), ptr(k),
                                                      C.c_int(capi.PROP_F32), C.c_int64(heads * d), ptr(v), C.c_int(capi.PROP_F32), C.c_int64(heads * dv),
                                                      C.c_int(d), C.c_int(dv), C.c_int(heads), C.c_double(0.37), ptr(o32), ptr(o64), C.c_int64(ldo), None,
                                                      ptr(y64), C.c_uint64(ycap), C.byref(st)))
    return st.as_dict()


def mixed_homes(engine, dev, row_ptr, nq, n, e, rng):
    """The C ABI takes each pointer on its own (the binding refuses what follows): q on the host, k and v on the device, out32 a
    host array and out64 a device tensor of one padded pitch, y64 on the host -- the bits of the all-host call, the padding kept"""
    heads, d, dv, fill = 2, 3, 2, -3.0
    w, ldo = heads * dv, heads * dv + 3
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    Q, K = ar.scores_operands(rng, nq, n, d, heads)
    V = rng.standard_normal((n, w)).astype(np.float32)
    Kd, Vd = torch.from_numpy(K).to(dev), torch.from_numpy(V).to(dev)
    for short in (256, 0):
        engine.set_option("attn_short", short)
        h32, h64, hy = np.full((nq, ldo), fill, np.float32), np.full((nq, ldo), fill, np.float64), np.zeros(heads * e, np.float64)
        hst = raw_attention(engine, rp, nq, Q, K, V, d, dv, heads, h32, h64, ldo, hy, heads * e)
        assert hst["q_on_device"] == hst["k_on_device"] == hst["v_on_device"] == 0 and hst["long_rows"] == (2 if short else nq - 1)
        m32, m64, my = np.full((nq, ldo), fill, np.float32), torch.full((nq, ldo), fill, dtype=torch.float64, device=dev), np.zeros(heads * e, np.float64)
        st = raw_attention(engine, rp, nq, Q, Kd, Vd, d, dv, heads, m32, m64, ldo, my, heads * e)
        assert st["q_on_device"] == 0 and st["k_on_device"] == st["v_on_device"] == 1, st
        g64 = m64.cpu().numpy()
        assert (m32[:, :w].view(np.uint32) == h32[:, :w].view(np.uint32)).all() and (g64[:, :w].view(np.uint64) == h64[:, :w].view(np.uint64)).all(), short
        assert (my.view(np.uint64) == hy.view(np.uint64)).all() and np.isfinite(h64[:, :w]).all() and (hy != 0).any(), short
        for pad in (m32[:, w:], g64[:, w:], h32[:, w:], h64[:, w:]):
            assert (pad == fill).all(), short
    engine.set_option("attn_short", 256)


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
    rng = np.random.Generator(np.random.PCG64(9900))
    # (d, dv, heads, first column of the slice inside a wider tensor): an aligned base with the widest loads, and bases and
    # pitches that allow only narrower ones
    for d, dv, heads, off in ((16, 8, 2, 0), (16, 8, 2, 1), (5, 6, 3, 2)):
        Q0, K0 = ar.scores_operands(rng, nq, n, d, heads)
        V0 = rng.standard_normal((n, heads * dv)).astype(np.float32)
        for bf16 in (False, True):
            if bf16:                                         # the values a bfloat16 tensor holds, as the twin reads them
                Qh, Kh, Vh = (pr.to_bf16_bits(x) for x in (Q0, K0, V0))
                mk = lambda bits_: torch.from_numpy(pr.widen_bf16(bits_).copy()).to(dev).to(torch.bfloat16)
            else:
                Qh, Kh, Vh = Q0, K0, V0
                mk = lambda x: torch.from_numpy(x).to(dev)
            wide = lambda t: torch.cat([torch.full((t.shape[0], off), float("nan"), dtype=t.dtype, device=dev), t,
                                        torch.full((t.shape[0], 3), float("nan"), dtype=t.dtype, device=dev)], dim=1)[:, off:off + t.shape[1]]
            Qd, Kd, Vd = (wide(mk(x)) for x in (Qh, Kh, Vh))
            assert Qd.stride(0) == heads * d + off + 3
            want = ar.attention_ref(row_ptr, ids, Qh, Kh, Vh, d, dv, heads, 0.37, bf16, bf16, bf16)
            for short in (256, 0):
                engine.set_option("attn_short", short)
                o32, o64, y32, y64, st = engine.sparse_attention(row_ptr, Qd, Kd, Vd, heads=heads, scale=0.37, want64=True, want_y32=True, want_y64=True)
                for x, dt, shape in ((o32, torch.float32, (nq, heads * dv)), (o64, torch.float64, (nq, heads * dv)), (y32, torch.float32, (heads, e)),
                                     (y64, torch.float64, (heads, e))):
                    assert x.is_cuda and x.device.index == engine.device and x.dtype == dt and tuple(x.shape) == shape
                assert (bits(o64) == want[0].view(np.uint64)).all() and (bits(o32) == want[1].view(np.uint32)).all(), (d, dv, heads, off, bf16, short)
                assert (bits(y64) == want[2].view(np.uint64)).all() and (bits(y32) == want[3].view(np.uint32)).all(), (d, dv, heads, off, bf16, short)
                assert st["q_on_device"] == st["k_on_device"] == st["v_on_device"] == 1 and st["nan_rows"] == 0
                # the same bits from host operands
                h32, h64, _, hy64, hst = engine.sparse_attention(row_ptr, Qh, Kh, Vh, heads=heads, scale=0.37, want64=True, want_y64=True,
                                                                 q_bf16=bf16, k_bf16=bf16, v_bf16=bf16)
                assert (h64.view(np.uint64) == want[0].view(np.uint64)).all() and (hy64.view(np.uint64) == want[2].view(np.uint64)).all()
                assert hst["q_on_device"] == hst["k_on_device"] == hst["v_on_device"] == 0
                # caller-made device outputs that are column slices of wider tensors keep their other columns
                t32 = torch.full((nq, heads * dv + 5), -3.0, dtype=torch.float32, device=dev)
                t64 = torch.full((nq, heads * dv + 5), -3.0, dtype=torch.float64, device=dev)
                engine.sparse_attention(row_ptr, Qd, Kd, Vd, heads=heads, scale=0.37, out32=t32[:, 2:2 + heads * dv], out64=t64[:, 2:2 + heads * dv])
                assert (bits(t64[:, 2:2 + heads * dv].contiguous()) == want[0].view(np.uint64)).all()
                assert (bits(t32[:, 2:2 + heads * dv].contiguous()) == want[1].view(np.uint32)).all()
                assert (t32[:, :2] == -3.0).all() and (t32[:, 2 + heads * dv:] == -3.0).all() and (t64[:, :2] == -3.0).all() and (t64[:, 2 + heads * dv:] == -3.0).all()
    mixed_homes(engine, dev, row_ptr, nq, n, e, rng)
    # mixed homes are refused by the binding
    try:
        engine.sparse_attention(row_ptr, Qd, K0, Vd, heads=heads)
    except ValueError:
        pass
    else:
        raise AssertionError("a host K beside device Q and V was accepted")
    engine.close()
    print("attention device ok")


if __name__ == "__main__":
    main()
