"""The host side of the top-k sparse rows (fora_amd/csrc/fora_topk_plan.h) checked on the CPU: tests/topk_plan_check.cpp
restates the plan by brute force -- held lengths, tiers, the chunking of a batch under "topk_cand", the clamping of the two
options, the stats sums -- and runs under the address and undefined-behaviour sanitizers.  The sanitized code is that
stand-alone program and nothing else.  The same file holds the twin (tests/sparse_topk_ref.py) against a plain Python sort."""
import os
import subprocess

import numpy as np
import pytest

from sparse_topk_ref import topk_csr, topk_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAX = 18432  # TOPK_LDS_MAX: the default and the upper bound of "topk_lds_cap"


@pytest.fixture(scope="session")
def topk_plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("topk") / "topk_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "topk_plan_check.cpp")], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    return r.stdout


def _plan(exe, k, lens, lds=LDS_MAX, cand=0, free=1 << 40, n=2000):
    words = _run(exe, "plan", k, lds, cand, free, n, ",".join(map(str, lens)) or "-").split()
    assert words[-1] == "ok"
    f = dict(w.split("=") for w in words[:-1])
    first = [] if f["first"] == "-" else [int(x) for x in f.pop("first").split(",")]
    f.pop("first", None)
    return {k_: int(v) for k_, v in f.items()}, first


def test_clamping_and_tier_boundaries(topk_plan_check):
    assert _run(topk_plan_check, "clamp").split() == ["ok"]


def test_bases_and_sums_above_2_32(topk_plan_check):
    assert _run(topk_plan_check, "wide").split() == ["ok"]


def test_held_lengths_and_tiers(topk_plan_check):
    lens = [0, 1, 63, 64, 65, 66, 2000, LDS_MAX, LDS_MAX + 1]
    for k in (1, 64, 10 ** 9):
        for lds in (0, 1, 64, LDS_MAX):
            f, _ = _plan(topk_plan_check, k, lens, lds=lds)
            assert f["held"] == sum(min(l, k) for l in lens)
            assert f["cut"] == sum(l > k for l in lens)
            assert f["lds"] == sum(k < l <= lds for l in lens) and f["global"] == sum(l > k and l > lds for l in lens)


def test_chunking(topk_plan_check):
    lens = [5, 0, 3, 9, 0, 0, 4, 4, 1]
    # topk_cand = 1: the scratch holds the longest row, and a row never shares a chunk unless it fits beside the others
    f, first = _plan(topk_plan_check, 2, [3, 3, 3, 3], cand=1)
    assert f["cap"] == 3 and first == [0, 1, 2, 3]                       # every row its own chunk
    f, first = _plan(topk_plan_check, 2, lens, cand=1)
    assert f["cap"] == 9 and first == [0, 3, 6]                          # 5 0 3 | 9 0 0 | 4 4 1 (rows of len 0 ride along)
    # a value that fits two or three rows
    f, first = _plan(topk_plan_check, 2, lens, cand=12)
    assert f["cap"] == 12 and first == [0, 3, 6]                         # 5 0 3 | 9 0 0 | 4 4 1
    f, first = _plan(topk_plan_check, 2, [4, 4, 4, 4, 4, 4, 4], cand=12)
    assert first == [0, 3, 6]                                            # three rows, three rows, one
    # 0: by free memory -- all of it, what is free, or the longest row when less is free
    f, first = _plan(topk_plan_check, 2, lens, cand=0, free=1 << 40)
    assert f["cap"] == sum(lens) and first == [0]
    f, first = _plan(topk_plan_check, 2, lens, cand=0, free=17)
    assert f["cap"] == 17 and first == [0, 6]                            # 5 0 3 9 0 0 | 4 4 1
    f, first = _plan(topk_plan_check, 2, lens, cand=0, free=2)
    assert f["cap"] == 9
    # a row longer than the option: the cap rises to it
    f, first = _plan(topk_plan_check, 2, [2, 50, 2, 2], cand=4)
    assert f["cap"] == 50 and first == [0, 1, 2]                         # 2 | 50 | 2 2
    # no rows, only empty rows; odd n: launches start on even rows (checked inside)
    f, first = _plan(topk_plan_check, 2, [])
    assert f["chunks"] == 0 and first == []
    f, first = _plan(topk_plan_check, 2, [0, 0, 0], cand=1)
    assert f["chunks"] == 1 and f["cap"] == 1
    for n in (2000, 2001):
        _plan(topk_plan_check, 2, [3, 3, 3, 3, 3], cand=1, n=n)
        _plan(topk_plan_check, 2, lens, cand=12, n=n)


def _sorted_ref(w, thr, k):
    """a plain Python sort by (word descending, id ascending)"""
    cand = [(int(x), v) for v, x in enumerate(w) if int(x) >= thr]
    if len(cand) > k:
        cand = sorted(cand, key=lambda t: (-t[0], t[1]))[:k]
    return sorted(v for _, v in cand)


def test_twin_against_a_plain_sort():
    rng = np.random.Generator(np.random.PCG64(77))
    for n, k in ((1, 1), (7, 3), (50, 1), (50, 49), (50, 50), (50, 51), (300, 64)):
        rows = [
            rng.integers(0, 5, size=n, dtype=np.uint64),                                  # few distinct words: ties on the k-th place
            np.full(n, 9, dtype=np.uint64),                                               # all equal
            rng.integers(0, 1 << 62, size=n, dtype=np.uint64),
            np.where(np.arange(n) % 3 == 0, np.uint64(1 << 62), np.uint64((1 << 62) + 5)),  # above 2^62: ~w must reverse the whole u64 order
            np.zeros(n, dtype=np.uint64),
        ]
        for w in rows:
            for thr in (1, 2, 1 << 61):
                assert list(topk_row(w, thr, k)) == _sorted_ref(w, thr, k), (n, k, thr)
    # ties: the lower ids win, and the result ascends by id
    w = np.array([5, 7, 5, 5, 9, 5], dtype=np.uint64)
    assert list(topk_row(w, 1, 3)) == [0, 1, 4] and list(topk_row(w, 1, 4)) == [0, 1, 2, 4] and list(topk_row(w, 6, 3)) == [1, 4]
    ptr, ids, fix, lens = topk_csr(np.stack([w, w[::-1]]), 1, 2)
    assert list(ptr) == [0, 2, 4] and list(ids) == [1, 4, 1, 4] and list(fix) == [7, 9, 9, 7] and list(lens) == [6, 6]
