"""Child process of tests/test_attention_bwd_gpu.py::test_device_operands_and_outputs: Engine.sparse_attention_bwd with the
operands and the outputs in device memory.  torch is imported first, so that the library binds to the HIP runtime torch brought
along and a tensor's data_ptr() is device memory the library knows.  The process starts fresh and ends here."""
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
import attention_bwd_ref as abr  # noqa: E402
import attention_ref as ar  # noqa: E402
import propagate_ref as pr  # noqa: E402

SEED = 0x464F5241


def bits(x):
    a = x.detach().cpu().contiguous().numpy()
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr() if torch.is_tensor(x) else x.ctypes.data)


def raw_attention_bwd(engine, rp, nq, q, k, v, g, y, d, dv, heads, outs, lds):
    """fora_hip_sparse_attention_bwd itself, every pointer as given (f32 operands, rows back to back, an f64 y); outs: dq32, dq64,
    dk32, dk64, dv32, dv64; lds: lddq, lddk, lddv; the stats"""
    gr, st = capi.AttnGrads(), capi.AttnBwdStats()
    for name, o in zip(("dq32", "dq64", "dk32", "dk64", "dv32", "dv64"), outs):
        setattr(gr, name, None if o is None else ptr(o).value)
    gr.lddq, gr.lddk, gr.lddv = lds
    f32 = C.c_int(capi.PROP_F32)
    engine._chk(engine._lib.fora_hip_sparse_attention_bwd(engine._ctx, ptr(rp), C.c_int(nq), ptr(q), f32, C.c_int64(heads * d), ptr(k), f32, C.c_int64(heads * d),
                                                          ptr(v), f32, C.c_int64(heads * dv), ptr(g), f32, C.c_int64(heads * dv), ptr(y), C.c_int(capi.PROP_F64),
                                                          C.c_uint64(y.shape[0]), C.c_int(d), C.c_int(dv), C.c_int(heads), C.c_double(0.37), C.byref(gr), C.byref(st)))
    return st.as_dict()


def mixed_homes(engine, dev, row_ptr, nq, n, e, rng):
    """The C ABI takes each pointer on its own (the binding refuses what follows): g and y on the device, q, k and v on the host;
    dq32 and dv32 host arrays, dk64 and dv64 device tensors, every pitch padded -- the bits of the all-host call, the padding kept"""
    heads, d, dv, fill = 2, 3, 2, -3.0
    wq, wv = heads * d, heads * dv
    lds = (wq + 3, wq + 2, wv + 3)
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    Q, K = ar.scores_operands(rng, nq, n, d, heads)
    V = rng.standard_normal((n, wv)).astype(np.float32)
    G = rng.standard_normal((nq, wv)).astype(np.float32)
    y = np.ascontiguousarray(engine.sparse_attention(row_ptr, Q, K, V, heads=heads, scale=0.37, want32=False, want64=True, want_y64=True)[3].reshape(heads * e))
    Gd, yd = torch.from_numpy(G).to(dev), torch.from_numpy(y).to(dev)
    host = lambda rows, ld, dt: np.full((rows, ld), fill, dt)
    for short in (256, 0):
        engine.set_option("attn_short", short)
        hq32, hk64, hv32, hv64 = host(nq, lds[0], np.float32), host(n, lds[1], np.float64), host(n, lds[2], np.float32), host(n, lds[2], np.float64)
        hst = raw_attention_bwd(engine, rp, nq, Q, K, V, G, y, d, dv, heads, (hq32, None, None, hk64, hv32, hv64), lds)
        assert all(hst[x + "_on_device"] == 0 for x in "qkvgy") and hst["long_rows"] > 0 and hst["long_cols"] > 0, hst
        assert (hst["short_rows"] > 0 and hst["short_cols"] > 0) == (short > 0), hst
        mq32, mv32 = host(nq, lds[0], np.float32), host(n, lds[2], np.float32)
        mk64 = torch.full((n, lds[1]), fill, dtype=torch.float64, device=dev)
        mv64 = torch.full((n, lds[2]), fill, dtype=torch.float64, device=dev)
        st = raw_attention_bwd(engine, rp, nq, Q, K, V, Gd, yd, d, dv, heads, (mq32, None, None, mk64, mv32, mv64), lds)
        assert st["q_on_device"] == st["k_on_device"] == st["v_on_device"] == 0 and st["g_on_device"] == st["y_on_device"] == 1, st
        for got, want, w in ((mq32, hq32, wq), (mk64.cpu().numpy(), hk64, wq), (mv32, hv32, wv), (mv64.cpu().numpy(), hv64, wv)):
            assert (bits(torch.from_numpy(got[:, :w].copy())) == bits(torch.from_numpy(want[:, :w].copy()))).all(), short
            assert np.isfinite(want[:, :w]).all() and (want[:, :w] != 0).any()
            assert (got[:, w:] == fill).all() and (want[:, w:] == fill).all(), short
    engine.set_option("attn_short", 256)


def main():
    assert torch.cuda.is_available()
    engine = fora_amd.Engine(0, lib=capi.TEST_LIB)          # the build with the row injection
    dev = torch.device("cuda", engine.device)
    n, m, row_ptr_g, col = synth.preset("tiny", "none")
    engine.set_graph(n, m, row_ptr_g, col)
    engine.set_params(epsilon=0.5, seed=SEED)
    rows_fix = abr.injected(n)
    row_ptr, _ = engine.test_sparse_rows(rows_fix, threshold=0.0)
    nq, e = rows_fix.shape[0], int(row_ptr[-1])
    ids = np.zeros(e, np.int32)
    engine.sparse_fetch(ids=ids, cap=e)
    rng = np.random.Generator(np.random.PCG64(9905))
    # (d, dv, heads, first column of the slice inside a wider tensor): an aligned base with the widest loads, and bases and
    # pitches that allow only narrower ones
    for d, dv, heads, off in ((16, 8, 2, 0), (16, 8, 2, 1), (5, 6, 3, 2)):
        Q0, K0 = ar.scores_operands(rng, nq, n, d, heads)
        V0 = rng.standard_normal((n, heads * dv)).astype(np.float32)
        G0 = rng.standard_normal((nq, heads * dv)).astype(np.float32)
        for bf16 in (False, True):
            if bf16:                                         # the values a bfloat16 tensor holds, as the twin reads them
                Qh, Kh, Vh, Gh = (pr.to_bf16_bits(x) for x in (Q0, K0, V0, G0))
                mk = lambda bits_: torch.from_numpy(pr.widen_bf16(bits_).copy()).to(dev).to(torch.bfloat16)
            else:
                Qh, Kh, Vh, Gh = Q0, K0, V0, G0
                mk = lambda x: torch.from_numpy(x).to(dev)
            wide = lambda t: torch.cat([torch.full((t.shape[0], off), float("nan"), dtype=t.dtype, device=dev), t,
                                        torch.full((t.shape[0], 3), float("nan"), dtype=t.dtype, device=dev)], dim=1)[:, off:off + t.shape[1]]
            Qd, Kd, Vd, Gd = (wide(mk(x)) for x in (Qh, Kh, Vh, Gh))
            assert Gd.stride(0) == heads * dv + off + 3
            for y64 in (False, True):
                _, _, y32d, y64d, _ = engine.sparse_attention(row_ptr, Qd, Kd, Vd, heads=heads, scale=0.37, want_y32=not y64, want_y64=y64)
                yd = y64d if y64 else y32d
                yh = yd.cpu().numpy()
                want = abr.attention_bwd_ref(row_ptr, ids, Qh, Kh, Vh, Gh, yh, n, d, dv, heads, 0.37, bf16, bf16, bf16, bf16)
                for short in (256, 0):
                    engine.set_option("attn_short", short)
                    r = engine.sparse_attention_bwd(row_ptr, Qd, Kd, Vd, Gd, yd, heads=heads, scale=0.37, want64=True)
                    st = r[6]
                    for i, (rows, w) in enumerate(((nq, heads * d), (n, heads * d), (n, heads * dv))):
                        for x, dt in ((r[2 * i], torch.float32), (r[2 * i + 1], torch.float64)):
                            assert x.is_cuda and x.device.index == engine.device and x.dtype == dt and tuple(x.shape) == (rows, w)
                        assert (bits(r[2 * i + 1]) == want[i].view(np.uint64)).all(), (d, dv, heads, off, bf16, y64, short, i)
                        assert (bits(r[2 * i]) == want[i].astype(np.float32).view(np.uint32)).all(), (d, dv, heads, off, bf16, y64, short, i)
                    assert st["q_on_device"] == st["k_on_device"] == st["v_on_device"] == st["g_on_device"] == st["y_on_device"] == 1
                    # the same bits from host operands
                    h = engine.sparse_attention_bwd(row_ptr, Qh, Kh, Vh, Gh, yh, heads=heads, scale=0.37, want32=False, want64=True,
                                                    q_bf16=bf16, k_bf16=bf16, v_bf16=bf16, g_bf16=bf16)
                    assert all((h[2 * i + 1].view(np.uint64) == want[i].view(np.uint64)).all() for i in range(3))
                    assert h[6]["q_on_device"] == h[6]["g_on_device"] == h[6]["y_on_device"] == 0
                    # caller-made device outputs that are column slices of wider tensors keep their other columns: the zeroing of
                    # the empty columns stays inside the slice
                    outs, wides = {}, []
                    for name, rows, w in (("dq", nq, heads * d), ("dk", n, heads * d), ("dv", n, heads * dv)):
                        t32 = torch.full((rows, w + 5), -3.0, dtype=torch.float32, device=dev)
                        t64 = torch.full((rows, w + 5), -3.0, dtype=torch.float64, device=dev)
                        outs[name + "32"], outs[name + "64"] = t32[:, 2:2 + w], t64[:, 2:2 + w]
                        wides.append((t32, t64, w))
                    engine.sparse_attention_bwd(row_ptr, Qd, Kd, Vd, Gd, yd, heads=heads, scale=0.37, **outs)
                    for i, (t32, t64, w) in enumerate(wides):
                        assert (bits(t64[:, 2:2 + w]) == want[i].view(np.uint64)).all() and (bits(t32[:, 2:2 + w]) == want[i].astype(np.float32).view(np.uint32)).all()
                        assert (t32[:, :2] == -3.0).all() and (t32[:, 2 + w:] == -3.0).all() and (t64[:, :2] == -3.0).all() and (t64[:, 2 + w:] == -3.0).all()
    engine.set_option("attn_short", 256)
    mixed_homes(engine, dev, row_ptr, nq, n, e, rng)
    # mixed homes are refused by the binding
    try:
        engine.sparse_attention_bwd(row_ptr, Qd, K0, Vd, Gd, yd, heads=heads)
    except ValueError:
        pass
    else:
        raise AssertionError("a host K beside device operands was accepted")
    engine.close()
    print("attention bwd device ok")


if __name__ == "__main__":
    main()
