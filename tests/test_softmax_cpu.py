"""The twin of the ROW SOFTMAX contract (tests/softmax_ref.py) against yardsticks that are not the twin -- the library's own
exp_def header compiled for the CPU, math.exp, math.fsum, torch autograd -- and the rows the contract names one by one.  The
check program (tests/softmax_exp_check.cpp) runs under the address and undefined-behaviour sanitizers; the sanitized code is
that stand-alone program and nothing else.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import softmax_ref as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


@pytest.fixture(scope="session")
def exp_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("softmax") / "softmax_exp_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "softmax_exp_check.cpp")], check=True)
    return exe


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_the_header_gives_the_twins_bits_on_the_grid(exp_check, tmp_path):
    grid = sm.exp_grid()
    assert grid.size > 4000 and (grid <= 0).all()
    for must in (0.0, -708.0, np.nextafter(-708.0, 0.0), np.nextafter(-708.0, -np.inf), -np.inf):
        assert (grid == must).any()
    assert np.signbit(grid[grid == 0.0]).any() and not np.signbit(grid[grid == 0.0]).all()      # both zeros
    path = tmp_path / "grid.txt"
    path.write_text("".join(f"{int(w):016x}\n" for w in _bits(grid)))
    r = subprocess.run([exp_check, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    got = np.array([int(line, 16) for line in r.stdout.split()], dtype=np.uint64)
    want = _bits(sm.exp_def(grid))
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(float(grid[i]).hex(), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]


def test_exp_def_edges():
    one = _bits(1.0)
    assert _bits(sm.exp_def(0.0)) == one and _bits(sm.exp_def(-0.0)) == one
    for t in (-np.inf, np.nextafter(-708.0, -np.inf), -709.0, -1e308):
        assert _bits(sm.exp_def(t)) == 0                                   # +0.0
    tiny = sm.exp_def(np.array([-708.0, np.nextafter(-708.0, 0.0)]))
    assert (tiny >= 2.0 ** -1022).all()                                    # the smallest results are normal
    grid = sm.exp_grid()
    e = sm.exp_def(grid)
    assert ((e == 0.0) | (e >= 2.0 ** -1022)).all() and (e <= 1.0).all() and not np.signbit(e).any()


def test_exp_def_is_within_2_ulp_of_math_exp():
    """1 ulp is exp_def's own error (measured: 1.0), the second is the libm's"""
    rng = np.random.Generator(np.random.PCG64(8720))
    grid = sm.exp_grid()
    pts = np.concatenate([grid[grid >= -708.0], -rng.random(20000) * 708.0, -rng.random(20000) * 2.0])
    got = sm.exp_def(pts)
    worst = 0.0
    for t, g in zip(pts.tolist(), got.tolist()):
        ref = math.exp(t)
        worst = max(worst, abs(g - ref) / math.ulp(ref))
    print(f"worst error against math.exp: {worst:.3f} ulp")
    assert worst <= 2.0


LENS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 600, 1000, 2049, 5000]


def _row_ptr(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_softmax_is_within_the_bound_of_the_stated_order(dtype):
    """against math.exp and math.fsum on the same x = scores * scale: exp's ulp, the 4 + 6 + (segments - 1) positive adds of
    the stated order, the division and some slack -- (ceil(len / 256) + 16) * 2^-53 relative, computed from len, not tuned"""
    rng = np.random.Generator(np.random.PCG64(8730))
    row_ptr = _row_ptr(LENS)
    for scale in (1.0, 0.37, -2.0):
        scores = ((rng.random(int(row_ptr[-1])) * 2 - 1) * 30).astype(dtype)
        out64, out32, nan_rows = sm.softmax_ref(row_ptr, scores, scale)
        assert nan_rows == 0 and (out32 == out64.astype(np.float32)).all()
        x = scores.astype(np.float64) * scale
        worst = 0.0
        for i, L in enumerate(LENS):
            xr = x[row_ptr[i]:row_ptr[i + 1]].tolist()
            m = max(xr)
            p = [math.exp(v - m) for v in xr]
            S = math.fsum(p)
            bound = (-(-L // 256) + 16) * U
            for e, pv in enumerate(p):
                ref = pv / S
                err = abs(float(out64[row_ptr[i] + e]) - ref) / ref
                worst = max(worst, err / bound)
                assert err <= bound, (L, e, err, bound)
        print(f"scale={scale}: worst error / bound = {worst:.3f}")


def test_backward_against_torch_autograd():
    """dx of the twin, fed torch's own f64 forward output, against autograd of torch_ops.row_softmax(scores * scale) in f64.
    In exact arithmetic both are (g_e - D) * y_e * scale, D = sum y g.  The twin's D carries the product's rounding and a
    chain of 4 + 6 + (segments - 1) adds: (segments + 10) u sum|y g|; the subtraction and the two multiplies add 3 u (|g_e| +
    sum|y g|).  Autograd sums in an order that is not ours -- at worst one entry after the other, (len - 1) adds -- and
    takes a handful of roundings per entry (exp, two divisions, the products): (len + 16) u on the same magnitude.  So
    |dx - dx_autograd| <= (segments + 13 + len + 16) * 2^-53 * (|g_e| + sum|y g|) * y_e * |scale|, computed from len."""
    import torch
    from fora_amd import torch_ops
    rng = np.random.Generator(np.random.PCG64(8740))
    row_ptr = _row_ptr([0] + LENS)
    for scale in (1.0, 0.37, -2.0):
        scores = (rng.random(int(row_ptr[-1])) * 2 - 1) * 30
        g = rng.standard_normal(scores.size)
        s_t = torch.tensor(scores, dtype=torch.float64, requires_grad=True)
        y_t = torch_ops.row_softmax(row_ptr, s_t * scale)
        y_t.backward(torch.tensor(g, dtype=torch.float64))
        want = s_t.grad.numpy()
        y = y_t.detach().numpy()
        got, got32 = sm.softmax_bwd_ref(row_ptr, y, g, scale)
        assert (got32 == got.astype(np.float32)).all()
        worst = 0.0
        for i in range(len(row_ptr) - 1):
            a, b = int(row_ptr[i]), int(row_ptr[i + 1])
            if a == b:
                continue
            L = b - a
            mass = math.fsum(np.abs(y[a:b] * g[a:b]))
            bound = (-(-L // 256) + 13 + L + 16) * U * (np.abs(g[a:b]) + mass) * y[a:b] * abs(scale)
            err = np.abs(got[a:b] - want[a:b])
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (L, float((err / bound).max()))
        print(f"scale={scale}: worst error / bound = {worst:.3f}")


def test_backward_types_widen_exactly():
    rng = np.random.Generator(np.random.PCG64(8750))
    row_ptr = _row_ptr([5, 0, 300])
    y32 = rng.random(305).astype(np.float32)
    g32 = rng.standard_normal(305).astype(np.float32)
    base, _ = sm.softmax_bwd_ref(row_ptr, y32.astype(np.float64), g32.astype(np.float64), 0.5)
    for y in (y32, y32.astype(np.float64)):
        for g in (g32, g32.astype(np.float64)):
            got, _ = sm.softmax_bwd_ref(row_ptr, y, g, 0.5)
            assert (_bits(got) == _bits(base)).all()


def test_special_rows():
    qnan = 0x7FF8000000000000
    inf = np.inf
    rows = {
        "nan": [1.0, np.nan, -3.0],
        "plus_inf": [1.0, inf, 2.0],
        "all_minus_inf": [-inf, -inf, -inf, -inf],
        "one_minus_inf": [0.5, -inf, 1.5, -2.0],
        "far_below": [0.0, -708.5, -709.0, -1.0, -707.0],
        "empty": [],
        "plain": [3.0, -1.0, 2.0],
        "zeros": [0.0, -0.0, 0.0],
    }
    names = list(rows)
    row_ptr = _row_ptr([len(rows[k]) for k in names])
    scores = np.array([v for k in names for v in rows[k]], dtype=np.float64)
    out64, out32, nan_rows = sm.softmax_ref(row_ptr, scores, 1.0)
    assert nan_rows == 3
    span = {k: slice(int(row_ptr[i]), int(row_ptr[i + 1])) for i, k in enumerate(names)}
    for k in ("nan", "plus_inf", "all_minus_inf"):
        assert (_bits(out64[span[k]]) == qnan).all() and (out32[span[k]].view(np.uint32) == 0x7FC00000).all()
    y = out64[span["one_minus_inf"]]
    assert _bits(y[1]) == 0 and (y[[0, 2, 3]] > 0).all()                   # +0.0 for the -inf entry
    y = out64[span["far_below"]]
    assert _bits(y[1]) == 0 and _bits(y[2]) == 0 and y[4] > 0 and y[4] >= 2.0 ** -1022
    assert (_bits(out64[span["zeros"]]) == _bits(1.0 / 3.0)).all()          # +0.0 and -0.0 alike: exp_def of either is 1.0
    for k in names:
        if k in ("nan", "plus_inf", "all_minus_inf", "empty"):
            continue
        y, x = out64[span[k]], scores[span[k]]
        assert ((y >= 0.0) & (y <= 1.0)).all()
        p = sm.exp_def(x - x.max())
        S = sm.row_sum(p)
        assert S >= 1.0 and _bits(y[int(np.argmax(x))]) == _bits(1.0 / S)   # the argmax entry is exactly 1 / S
    # scale = 0: every finite score becomes +-0.0 -- a uniform row; a non-finite one becomes NaN and takes its row with it
    o0, _, n0 = sm.softmax_ref(row_ptr, scores, 0.0)
    assert n0 == 4
    for k in ("nan", "plus_inf", "all_minus_inf", "one_minus_inf"):
        assert (_bits(o0[span[k]]) == qnan).all()
    assert (_bits(o0[span["far_below"]]) == _bits(1.0 / 5.0)).all() and (_bits(o0[span["plain"]]) == _bits(1.0 / 3.0)).all()
    # a NaN row touches no other row
    assert not np.isnan(out64[span["plain"]]).any()


def test_the_sum_is_cut_every_256_entries_and_lane_ordered():
    """the order is the contract: terms that a plain left-to-right sum and the stated order add differently"""
    t = np.array([1.0] + [2.0 ** -53] * 64, dtype=np.float64)
    # lane 0 adds 1 + u = 1 (a tie, to even) and the tree's first step 1 + u = 1 again; the other 62 u meet each other first and
    # arrive as 2 u, 4 u, ... 32 u, each exact on top of 1: 1 + 62 u.  One entry after the other would have stayed at 1.
    assert sm.row_sum(t) == 1.0 + 62 * 2.0 ** -53
    big = np.ones(600)
    assert sm.row_sum(big) == 600.0
    st = sm.softmax_stats_ref(_row_ptr(sm.ROW_LENS))
    assert st == {"entries": sum(sm.ROW_LENS), "segments": 1 * 7 + 2 + 3 + 1, "max_row": 600, "short_rows": 8, "long_rows": 2}
    assert sm.softmax_stats_ref(_row_ptr(sm.ROW_LENS), 0)["long_rows"] == 10 and sm.softmax_stats_ref(_row_ptr(sm.ROW_LENS), 64)["short_rows"] == 5


@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("softmax_plan") / "softmax_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "softmax_plan_check.cpp")], check=True)
    return exe


def test_the_work_lists_against_brute_force(plan_check):
    """fora_softmax_plan.h: every entry in exactly one list, a long row's segments consecutive behind their `slot`"""
    rng = np.random.Generator(np.random.PCG64(8760))
    cases = [sm.ROW_LENS, [], [0, 0], [256], [257], [1, 600, 1, 26140, 0, 64], [int(x) for x in rng.integers(0, 900, size=40)]]
    for lens in cases:
        for option in (256, 0, 1, 64, 255, 1000, -5):
            arg = ",".join(map(str, lens)) or "-"
            r = subprocess.run([plan_check, str(option), arg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0 and not r.stderr, (option, lens, r.stdout[-500:], r.stderr[-2000:])
            st = sm.softmax_stats_ref(_row_ptr(lens), option)
            segs = {True: 0, False: 0}
            cap = min(max(option, 0), 256)
            for L in lens:
                segs[L <= cap] += -(-L // 256)
            assert r.stdout.split() == [f"short={segs[True]}", f"long={segs[False]}", f"short_rows={st['short_rows']}", f"long_rows={st['long_rows']}", "ok"]


def test_abi_surface():
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    assert "ROW SOFTMAX" in hdr and "fora_hip_test_exp" in hdr
    assert capi.STRUCTS["fora_softmax_stats"] is capi.SoftmaxStats  # (its fields and size against the header: tests/test_capi_cpu.py)
    product, test = capi.load(), capi.load(capi.TEST_LIB)
    for name in ("fora_hip_sparse_softmax", "fora_hip_sparse_softmax_bwd"):
        assert hasattr(product, name) and hasattr(test, name) and name in capi.SYMBOLS
    assert hasattr(test, "fora_hip_test_exp") and not hasattr(product, "fora_hip_test_exp")
    # NULL ctx: answered without touching the GPU
    assert product.fora_hip_sparse_softmax(None, None, 0, None, 0, 1.0, None, None, 0, None) == -1
    assert product.fora_hip_sparse_softmax_bwd(None, None, 0, None, 0, None, 0, 1.0, None, None, 0, None) == -1
    assert test.fora_hip_test_exp(None, None, 0, None) == -1
    for meth in ("sparse_softmax", "sparse_softmax_bwd", "test_exp"):
        assert callable(getattr(capi.Engine, meth))
