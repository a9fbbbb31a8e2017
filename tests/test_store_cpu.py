"""The host side of the ROW STORE (fora_amd/csrc/fora_store_plan.h) checked on the CPU: tests/store_plan_check.cpp restates the
take plan by brute force -- every output entry maps to its (row, place), every span's window starts at the row of its first
entry -- and runs under the address and undefined-behaviour sanitizers.  The sanitized code is that stand-alone program and
nothing else.  The numpy twin (tests/store_ref.py) and the boundary (header, library, capi.SYMBOLS) are checked here too."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import store_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [0, 1, 63, 64, 65, 127, 128, 129, 256, 257, 2000]
NAMES = ["fora_hip_store_put", "fora_hip_store_load", "fora_hip_store_take", "fora_hip_store_info", "fora_hip_store_clear"]


@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("store") / "store_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "store_plan_check.cpp")], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    return r.stdout.split()


def _join(xs):
    return ",".join(map(str, xs)) or "-"


def _take(exe, span, lens, rows):
    out = _run(exe, "take", span, _join(lens), _join(rows))
    assert out[-1] == "ok", out
    f = {k: int(v) for k, v in (w.split("=") for w in out[:-1])}
    assert f["entries"] == sum(lens[r] for r in rows)
    return f


@pytest.mark.parametrize("span", [64, 256])
def test_every_length_in_every_order(plan_check, span):
    R = len(LENS)
    rng = np.random.Generator(np.random.PCG64(11))
    for rows in (list(range(R)), list(range(R))[::-1], list(rng.permutation(R)), [10, 10, 3, 3, 3, 0, 4], [r for r in range(R) for _ in range(2)]):
        f = _take(plan_check, span, LENS, rows)
        assert f["spans"] == -(-f["entries"] // span)
    for L in LENS:                                        # each length alone, twice, and between two rows of one entry
        _take(plan_check, span, [L], [0])
        _take(plan_check, span, [L], [0, 0])
        _take(plan_check, span, [1, L, 1], [0, 1, 2])


@pytest.mark.parametrize("span", [64, 256])
def test_empty_cases(plan_check, span):
    assert _take(plan_check, span, LENS, [])["spans"] == 0                    # nb == 0
    assert _take(plan_check, span, [], [])["spans"] == 0                      # ... of an empty store
    assert _take(plan_check, span, [0, 0, 0], [0, 1, 2, 1])["spans"] == 0     # all rows empty
    lens = [0, 0, 70, 0, 0, 0, 64, 0, 1, 0, 0]
    _take(plan_check, span, lens, list(range(len(lens))))                     # leading, consecutive and trailing empty rows
    _take(plan_check, span, lens, [0, 1, 3, 2, 4, 5, 9, 10])
    f = _take(plan_check, span, [span] + [0] * 700 + [span], list(range(702)))  # a window of 702 rows: past what the kernels stage
    assert f["max_win"] == 702 and f["spans"] == 2


def test_bad_take_index_is_rejected(plan_check):
    R = len(LENS)
    assert _run(plan_check, "take", 64, _join(LENS), "0,-1,2") == ["rejected", "1"]
    assert _run(plan_check, "take", 64, _join(LENS), f"0,1,{R}") == ["rejected", "2"]
    assert _run(plan_check, "take", 64, _join(LENS), f"{R},-1") == ["rejected", "0"]
    assert _run(plan_check, "take", 64, "-", "0") == ["rejected", "0"]          # R on an empty store


def test_bad_row_ptr_is_rejected(plan_check):
    for good in ("0", "0,0", "0,3,3,9"):
        assert _run(plan_check, "rowptr", good) == ["ok"]
    for bad in ("1,2", "0,5,4", "0,-1", "-2,0", "0,3,2,9"):                      # non-zero start, decreasing, negative
        assert _run(plan_check, "rowptr", bad) == ["rejected"]


def test_span_option_is_a_multiple_of_64_at_least_64(plan_check):
    got = [int(_run(plan_check, "span", v)[0]) for v in (-5, 0, 1, 64, 100, 128, 2048, 2049, 1 << 40)]
    assert got == [64, 64, 64, 64, 64, 128, 2048, 2048, 65536]


def test_twin_take_and_load_rules():
    row_ptr = np.array([0, 2, 2, 5], dtype=np.int64)
    ids = np.array([4, 9, 1, 2, 7], dtype=np.int32)
    fix = np.array([0, 1, 2**64 - 1, 5, 1 << 62], dtype=np.uint64)
    rp, i, f, v = store_ref.take(row_ptr, ids, fix, [2, 1, 0, 2])
    assert list(rp) == [0, 3, 3, 5, 8] and list(i) == [1, 2, 7, 4, 9, 1, 2, 7]
    assert list(f) == [2**64 - 1, 5, 1 << 62, 0, 1, 2**64 - 1, 5, 1 << 62] and v[2] == 1.0 and v[0] == 4.0
    assert store_ref.take(row_ptr, ids, fix, [])[0].tolist() == [0]
    with pytest.raises(IndexError):
        store_ref.take(row_ptr, ids, fix, [3])
    assert store_ref.load_ok(row_ptr, ids, 10)                                # 9 then 1 across a row boundary is legal
    assert store_ref.first_bad_entry(row_ptr, ids, 9) == 1                    # id == n
    assert store_ref.first_bad_entry(row_ptr, [4, 4, 1, 2, 7], 10) == 1       # equal inside a row
    assert store_ref.first_bad_entry(row_ptr, [4, 9, 2, 1, 7], 10) == 3       # descending inside a row
    assert store_ref.first_bad_entry(row_ptr, [4, 9, -1, 2, 7], 10) == 2
    assert not store_ref.row_ptr_ok([1, 2]) and not store_ref.row_ptr_ok([0, 2, 1])
    a = store_ref.append((row_ptr, ids, fix), (row_ptr, ids, fix))
    assert a[0].tolist() == [0, 2, 2, 5, 7, 7, 10] and a[1].size == 10


def test_header_library_and_binding_name_the_store():
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fora_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fora_hip_\w+)\s*\(", text))
    lib = capi.load()
    for name in NAMES:
        assert name in declared and hasattr(lib, name) and name in capi.SYMBOLS, name
    assert "fora_store_stats" in text and capi.STRUCTS["fora_store_stats"] is capi.StoreStats  # (fields, size: tests/test_capi_cpu.py)
    for m in ("store_put", "store_load", "store_take", "store_info", "store_clear"):
        assert callable(getattr(capi.Engine, m))
    # a NULL ctx is answered without touching the GPU (there is none here)
    one = (ctypes.c_int64 * 2)()
    assert lib.fora_hip_store_put(None, one, 0, 0, None) == -1
    assert lib.fora_hip_store_load(None, one, 0, None, None, 0, None) == -1
    assert lib.fora_hip_store_take(None, one, 0, one, None) == -1
    assert lib.fora_hip_store_info(None, None, None, None) == -1
    assert lib.fora_hip_store_clear(None) == -1
    assert "take_span" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
