"""The arithmetic of COLUMNS (fora_amd/csrc/fora_cols_plan.h) checked on the CPU: tests/cols_plan_check.cpp restates mark, totals,
scan, list and relabel on the host through the header's functions, holds them to brute force, and runs under the address and
undefined-behaviour sanitizers.  The sanitized code is that stand-alone program and nothing else.  The numpy twin
(tests/cols_ref.py) and the boundary (header, library, capi.SYMBOLS) are checked here too."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cols_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 63, 64, 65, 127, 128, 129, 2000, 32000]
BLOCKS = [1, 4, 256]
NAMES = ["fora_hip_sparse_compact", "fora_hip_sparse_cols_fetch"]


@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cols") / "cols_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cols_plan_check.cpp")], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    return r.stdout.split()


def _join(xs):
    return ",".join(map(str, xs)) or "-"


def _compact(exe, n, block, ids):
    out = _run(exe, "compact", n, block, _join(ids))
    assert out[-1] == "ok", out
    return {k: int(v) for k, v in (w.split("=") for w in out[:-1])}


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("n", NS)
def test_the_id_sets_every_n_must_survive(plan_check, n, block):
    """empty, a single id, {0, n - 1}, every id, every 64th id, both sides of each word boundary: inside the program"""
    out = _run(plan_check, "sets", n, block)
    assert out[-1] == "ok" and int(out[0].split("=")[1]) >= 10, out


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("n", NS)
def test_random_ids_against_the_twin(plan_check, n, block):
    rng = np.random.Generator(np.random.PCG64(n * 7 + block))
    for count in (1, 5, 64, 700):
        ids = rng.integers(0, n, size=count)
        f = _compact(plan_check, n, block, ids)
        cols, local = cols_ref.compact(ids)
        assert f["nc"] == cols.size and f["words"] == -(-n // 64) and f["blocks"] == -(-f["words"] // block)
        assert np.array_equal(cols[local], ids.astype(np.int32))


def test_block_option_is_a_power_of_two_from_1_to_4096(plan_check):
    got = [int(_run(plan_check, "block", v)[0]) for v in (-5, 0, 1, 2, 3, 4, 255, 256, 257, 1024, 4095, 4096, 4097, 1 << 40)]
    assert got == [1, 1, 1, 2, 2, 4, 128, 256, 256, 1024, 2048, 4096, 4096, 4096]


def test_twin_rules():
    cols, local = cols_ref.compact([7, 3, 7, 0, 1999, 3])
    assert cols.dtype == np.int32 and local.dtype == np.int32
    assert cols.tolist() == [0, 3, 7, 1999] and local.tolist() == [2, 1, 2, 0, 3, 1]
    cols, local = cols_ref.compact([])
    assert cols.size == 0 and local.size == 0 and cols.dtype == np.int32
    ids = np.arange(50, dtype=np.int32)                       # every id: the identity
    cols, local = cols_ref.compact(ids)
    assert np.array_equal(cols, ids) and np.array_equal(local, ids)
    row = np.array([2, 9, 40, 41], dtype=np.int32)            # monotone: ascending ids stay strictly ascending
    _, local = cols_ref.compact(np.concatenate([row, [5, 41, 100]]))
    assert np.all(np.diff(local[:4]) > 0)


def test_header_library_and_binding_name_the_columns():
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fora_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fora_hip_\w+)\s*\(", text))
    lib = capi.load()
    for name in NAMES:
        assert name in declared and hasattr(lib, name) and name in capi.SYMBOLS, name
    assert "fora_cols_stats" in text and capi.STRUCTS["fora_cols_stats"] is capi.ColsStats  # (fields, size: tests/test_capi_cpu.py)
    for m in ("sparse_compact", "store_take_compact"):
        assert callable(getattr(capi.Engine, m))
    assert isinstance(capi.Engine.held_cols, property)
    # a NULL ctx is answered without touching the GPU (there is none here)
    one = (ctypes.c_int64 * 2)()
    assert lib.fora_hip_sparse_compact(None, one, 0, one, None) == -1
    assert lib.fora_hip_sparse_cols_fetch(None, None, 0) == -1
    assert "cols_block" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
