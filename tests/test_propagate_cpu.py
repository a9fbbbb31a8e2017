"""PROPAGATE (fora_hip_sparse_propagate) without a GPU: the numpy twin (tests/propagate_ref.py) against an independent
yardstick, the test inputs' power to tell one order of additions from another, the host-only segment plan
(fora_amd/csrc/fora_prop_plan.h) against brute force under the address and undefined-behaviour sanitizers -- a stand-alone
program and nothing else is sanitized -- and the library's symbol."""
import math
import os
import subprocess

import numpy as np
import pytest

import propagate_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX_ONE = 1 << 62


def _row(rng, n, length):
    """a row of `length` entries over n nodes: ids ascending, words random in [1, 2^62 / length]"""
    ids = np.sort(rng.choice(n, size=length, replace=False)).astype(np.int32)
    fix = rng.integers(1, FIX_ONE // max(length, 1) + 1, size=length, dtype=np.uint64)
    return ids, fix


def _rows(rng, n, lens):
    parts = [_row(rng, n, L) for L in lens]
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return row_ptr, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@pytest.mark.parametrize("bf16", [False, True])
def test_twin_against_fsum(bf16):
    """(a) every output within len * 2^-52 * sum|term| of the exactly rounded sum (math.fsum) of the same terms"""
    rng = np.random.Generator(np.random.PCG64(5100))
    n, d = 1200, 5
    lens = [0, 1, 2, 255, 256, 257, 513, 1000]
    row_ptr, ids, fix = _rows(rng, n, lens)
    H = pr.scaled_features(rng, n, d)
    if bf16:
        H = pr.to_bf16_bits(H)
    out64, out32 = pr.propagate_ref(row_ptr, ids, fix, H, bf16=bf16)
    H64 = (pr.widen_bf16(H) if bf16 else H).astype(np.float64)
    for i, L in enumerate(lens):
        lo, hi = int(row_ptr[i]), int(row_ptr[i + 1])
        terms = pr.row_terms(ids[lo:hi], fix[lo:hi], H64)
        for c in range(d):
            exact = math.fsum(terms[:, c])
            bound = L * 2.0 ** -52 * math.fsum(np.abs(terms[:, c]))
            assert abs(out64[i, c] - exact) <= bound, (L, c, out64[i, c], exact, bound)
    assert (out32 == out64.astype(np.float32)).all()
    assert (out64[0] == 0.0).all() and not np.signbit(out64[0]).any()          # an empty row: +0.0
    # normalised: one division by the row's word sum
    norm64, _ = pr.propagate_ref(row_ptr, ids, fix, H, normalize=True, bf16=bf16)
    for i, L in enumerate(lens):
        S = sum(int(x) for x in fix[row_ptr[i]:row_ptr[i + 1]])
        want = out64[i] / math.ldexp(float(S), -62) if S else out64[i]
        assert (norm64[i] == want).all()


def test_bf16_widening_is_exact():
    bits = np.arange(0, 1 << 16, dtype=np.uint32).astype(np.uint16)
    f = pr.widen_bf16(bits)
    assert (f.view(np.uint32) == bits.astype(np.uint32) << 16).all()
    assert (pr.to_bf16_bits(f) == bits).all()


@pytest.mark.parametrize("length", [513, 1000])
def test_inputs_tell_the_orders_apart(length):
    """(b) over d = 64 columns the contract's sum differs in at least one word from the same terms added with segments of
    128, without segments, and by np.sum: a kernel that adds in another order cannot pass the bitwise tests"""
    rng = np.random.Generator(np.random.PCG64(5200 + length))
    n, d = 1500, 64
    ids, fix = _row(rng, n, length)
    H = pr.scaled_features(rng, n, d)
    terms = pr.row_terms(ids, fix, H.astype(np.float64))
    want = pr.sum_row(terms)
    differ = {"seg128": int((pr.sum_row(terms, 128) != want).sum()), "plain": int((pr.sum_row(terms, None) != want).sum()),
              "np.sum": int((np.sum(terms, axis=0) != want).sum())}
    print(length, differ)
    assert all(v >= 1 for v in differ.values()), differ
    # float32 outputs round the differences away far too often to carry a bit-order assertion: they are checked as (float)out64
    twin64, twin32 = pr.propagate_ref(np.array([0, length]), ids, fix, H)
    assert (twin64[0] == want).all() and (twin32[0] == want.astype(np.float32)).all()


def test_257_entries_test_the_boundary_not_the_order():
    """the second segment of a row of 257 entries holds one term: P_0 + (0.0 + t) is the plain sum"""
    rng = np.random.Generator(np.random.PCG64(5300))
    ids, fix = _row(rng, 1500, 257)
    terms = pr.row_terms(ids, fix, pr.scaled_features(rng, 1500, 64).astype(np.float64))
    assert (pr.sum_row(terms) == pr.sum_row(terms, None)).all()


# ---- (c) the host-only plan
@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prop") / "prop_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "prop_plan_check.cpp")], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    return r.stdout


def _plan(exe, option, lens, free_bytes=0, d=64):
    words = _run(exe, "plan", option, free_bytes, d, ",".join(map(str, lens)) or "-").split()
    assert words[-1] == "ok"
    return {k: int(v) for k, v in (w.split("=") for w in words[:-1])}


PLAN_ROWS = [
    [],
    [0], [0, 0, 0], [1], [256], [257], [512],
    [0, 1, 256, 257, 512, 0, 0],                 # empty, single-entry and boundary rows; trailing empty rows
    [0, 0, 513, 0, 1000, 1, 0, 255, 2000, 0],
    [300] * 7,
]


@pytest.mark.parametrize("option", [1, 3, 0])
def test_segment_plan_against_brute_force(plan_check, option):
    for lens in PLAN_ROWS:
        segs = sum((L + 255) // 256 for L in lens)
        # option 0: by free memory -- here room for two segments' partial sums (a table longer than one chunk), and plenty
        for free_bytes in ((2 * 4 * (64 * 8 + 8), 1 << 30) if option == 0 else (0,)):
            f = _plan(plan_check, option, lens, free_bytes)
            per = option if option else (2 if free_bytes < (1 << 30) else max(segs, 1))
            per = min(per, max(segs, 1))
            assert f["segments"] == segs and f["per"] == per
            assert f["chunks"] == (max(1, -(-segs // per)) if lens else 0)
            assert f["max_row"] == max(lens, default=0) and f["entries"] == sum(lens)
    assert _plan(plan_check, 3, [0, 1, 256, 257, 512, 0, 0])["chunks"] == 2 and _plan(plan_check, 1, [1000])["chunks"] == 4


def test_row_ptr_validation_and_lane_geometry(plan_check):
    assert _run(plan_check, "rowptr").split() == ["ok"]
    assert _run(plan_check, "geom").split()[-1] == "ok"


def test_driver_helpers_against_brute_force(plan_check):
    """the vector widths, the group exponent, the byte extents of the operands and the long-row segment count, each against
    a restatement at its edges"""
    assert _run(plan_check, "helpers").split()[-1] == "ok"


# ---- (d) the symbol
def test_symbol_and_null_ctx():
    """the library exports fora_hip_sparse_propagate and answers a NULL ctx with FORA_E_ARG without touching a GPU; the
    test entry point is in the test library only"""
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    assert "fora_hip_sparse_propagate" in capi.SYMBOLS
    product, test = capi.load(), capi.load(capi.TEST_LIB)
    for lib in (product, test):
        fn = lib.fora_hip_sparse_propagate
        rp = np.zeros(2, dtype=np.int64)
        out = np.full(4, 7.0, dtype=np.float32)
        assert fn(None, rp.ctypes.data, 1, None, 0, 4, 4, 0, out.ctypes.data, None, 4, None) == -1
        assert (out == 7.0).all()
    assert hasattr(test, "fora_hip_test_sparse_rows") and not hasattr(product, "fora_hip_test_sparse_rows")
    assert test.fora_hip_test_sparse_rows(None, None, 0, 0.0, None, None) == -1
    hdr = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    assert "fora_hip_test_sparse_rows" in hdr and "fora_hip_test_sparse_rows" not in __import__("re").sub(r"/\*.*?\*/", "", hdr, flags=__import__("re").S)
    for meth in ("sparse_propagate", "propagate", "propagate_seeds", "test_sparse_rows"):
        assert callable(getattr(capi.Engine, meth))
    assert capi.STRUCTS["fora_prop_stats"] is capi.PropStats  # (its fields and size against the header: tests/test_capi_cpu.py)
