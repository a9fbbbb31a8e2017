"""The row layout of the held results (fora_amd/csrc/fora_rows.h) checked on the CPU: tests/rows_check.cpp restates the
contract by brute force -- a dangling row is one entry, a live row its held length, row_ptr the prefix sum in the caller's
order -- and runs, under the address and undefined-behaviour sanitizers, on the smallest cases that can go wrong.  The
sanitized code is that stand-alone program and nothing else."""
import math
import os
import subprocess

import numpy as np
import pytest

from test_sparse_gpu import thr_fix_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def rows_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rows") / "rows_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "rows_check.cpp")], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    return r.stdout


def _layout(exe, rows, batches, max_size=0, sources=True):
    """rows: "d<source>" or a support length per row; batches: live rows per batch.  The facts of a passing run, row_ptr
    as a list -- held against the prefix sum computed here as well."""
    join = lambda xs: ",".join(map(str, xs)) or "-"
    words = _run(exe, "layout", max_size, ("" if sources else "*") + join(rows), join(batches)).split()
    assert words[-1] == "ok"
    f = dict(w.split("=") for w in words[:-1])
    row_ptr = [int(x) for x in f.pop("row_ptr").split(",")]
    f = {k: int(v) for k, v in f.items()}
    held = [1 if str(r).startswith("d") else (min(int(r), max_size) if max_size > 0 else int(r)) for r in rows]
    assert row_ptr == [0] + list(np.cumsum(held, dtype=np.int64)) and f["cur"] == row_ptr[-1]
    assert f["batches"] == len(batches) and f["dangling"] == sum(str(r).startswith("d") for r in rows)
    return f, row_ptr


def _splits(nlive):
    """batches of 1 row, of uneven sizes, and one batch for all rows"""
    out = [[1] * nlive, [nlive]] if nlive else [[]]
    if nlive >= 3:
        out += [[1, nlive - 1], [nlive - 2, 2], [2, 1] + [nlive - 3] * (nlive > 3)]
    return [b for i, b in enumerate(out) if b not in out[:i]]


def test_no_rows_and_only_dangling_rows(rows_check):
    f, row_ptr = _layout(rows_check, [], [])
    assert row_ptr == [0] and f["max_row"] == 0 and f["written"] == 0
    f, row_ptr = _layout(rows_check, ["d5", "d9", "d5"], [])
    assert row_ptr == [0, 1, 2, 3] and f["max_row"] == 1 and f["support"] == 3 and f["written"] == 0


def test_dangling_rows_first_between_inside_and_last(rows_check):
    # test_several_batches_with_a_dangling_row_between_them: live rows 0 1 | 3 4 | 5 7, row 2 between two batches, row 6 inside one, row 8 last
    rows = [4, 7, "d11", 3, 9, 2, "d12", 4, "d11"]
    f, row_ptr = _layout(rows_check, rows, [2, 2, 2])
    assert row_ptr == [0, 4, 11, 12, 15, 24, 26, 27, 31, 32] and f["max_row"] == 9 and f["written"] == 31
    # ... and dangling rows first; every split of the six live rows
    for lead in ([], ["d3"], ["d3", "d4"]):
        for b in _splits(6):
            _layout(rows_check, lead + rows, b)


def test_empty_rows_and_a_source_twice(rows_check):
    """a live row of length 0 (first, between, last, next to a dangling row); the same source live twice, and dangling twice"""
    for rows in ([0], [0, 0, 0], [0, 5, 0], [5, 0, "d1", 0], ["d1", 0, "d1"], [6, 6, 3, 6], [0, "d2", "d2", 0, 4]):
        nlive = sum(not str(r).startswith("d") for r in rows)
        for b in _splits(nlive):
            f, _ = _layout(rows_check, rows, b)
            assert f["max_row"] == max([1 if str(r).startswith("d") else r for r in rows])


@pytest.mark.parametrize("max_size", [1, 3])
def test_held_length_shorter_than_support(rows_check, max_size):
    rows = [0, 1, 5, "d8", 5, 1, 0]
    for b in _splits(6):
        f, row_ptr = _layout(rows_check, rows, b, max_size=max_size)
        assert f["max_row"] == 5 and f["support"] == 13                      # the supports, not what is held of them
        assert row_ptr[-1] == (5 if max_size == 1 else 9)


def test_identity_order_without_sources(rows_check):
    rows = [3, 0, 8, 1, 1, 6, 2]
    for b in ([1] * 7, [3, 3, 1], [7]):
        for max_size in (0, 3):
            f, _ = _layout(rows_check, rows, b, max_size=max_size, sources=False)
            assert f["dangling"] == 0 and f["max_row"] == 8
    _layout(rows_check, [], [], sources=False)


def test_geometry(rows_check):
    assert _run(rows_check, "geometry", 0).split() == ["cases=9", "ok"]    # 0: the kernels' SP_TILE (fora_consts.h)
    assert _run(rows_check, "geometry", 64).split() == ["cases=9", "ok"]


def test_growth_guess(rows_check):
    assert _run(rows_check, "growth").split()[-1] == "ok"


def test_threshold_word(rows_check):
    eps = 2.0 ** -62
    ts = [0.0, -1.0, -0.0, eps, math.nextafter(eps, 1.0), 1.0 / 3, 1e-3, 1.0]
    out = _run(rows_check, "threshold", *[t.hex() for t in ts], math.nextafter(1.0, 2.0).hex(), "nan", "inf").split()
    assert out[:len(ts)] == [str(thr_fix_of(t)) for t in ts]
    assert out[len(ts):] == ["rejected"] * 3
    assert [int(x) for x in out[:5]] == [1, 1, 1, 1, 2] and int(out[len(ts) - 1]) == 1 << 62
