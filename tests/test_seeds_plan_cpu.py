"""The planning of a seed-set call (fora_amd/csrc/fora_seeds_plan.h) checked on the CPU: tests/seeds_plan_check.cpp restates
the SEED SETS rules by brute force -- the checks of the sets, the weights at 2^-62 against tests/seeds_ref.py word for word,
slots in order of first appearance, the use list of every batch and the dangling seeds' terms decoded through the views the
library hands its kernels, the chunk of rows and the grid of k_seed_combine -- and runs, under the address and
undefined-behaviour sanitizers, on the smallest cases that can go wrong.  The sanitized code is that stand-alone program and
nothing else."""
import os
import subprocess

import pytest

import seeds_ref as sr
from test_seeds_cpu import EXACT, ROUNDED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def seeds_plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("seeds_plan") / "seeds_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "seeds_plan_check.cpp")], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    return r.stdout


def test_set_checks_answer_in_order(seeds_plan_check):
    """each refusal with its text; a call with two faults gets the earlier one"""
    run = lambda ns, ptr, seeds: _run(seeds_plan_check, "sets", ns, ptr, seeds).strip()
    assert run(-1, "null", "null") == "bad sets: negative count"
    assert run(0, "null", "null") == "fine"                                    # nothing is read
    assert run(1, "null", "3") == run(1, "0,1", "null") == "bad sets: null set_ptr or seeds"
    assert run(2, "1,0,0", "3") == "set_ptr[0] must be 0"                      # ... before the sets are looked at
    assert run(2, "0,2,1", "3,4") == "set_ptr decreases"
    assert run(2, "0,1,1", "3") == run(2, "0,0,1", "3") == "empty seed set"
    assert run(3, "0,1,1,0", "3") == "empty seed set"                          # the first bad set answers
    assert run(2, "0,1,2147483648", "3") == "more than 2^31 - 1 seeds in one call"   # (the seeds are not read)
    assert run(2, "0,1,2147483647", "3") == run(2, "0,2,3", "3,4,3") == "fine"


@pytest.mark.parametrize("k", [1, 2, 3, 7, 1000])
def test_uniform_words_equal_the_twin(seeds_plan_check, k):
    assert [int(x) for x in _run(seeds_plan_check, "uniform", k).split()] == sr.uniform_wfix(k)


@pytest.mark.parametrize("weights", EXACT + ROUNDED)
def test_weighted_words_equal_the_twin(seeds_plan_check, weights):
    out = _run(seeds_plan_check, "weights", *[float(w).hex() for w in weights]).split()
    assert [int(x) for x in out] == sr.weighted_wfix(weights)


@pytest.mark.parametrize("bad,text", [([-1.0, 2.0], "seed weights must be finite and >= 0"), ([float("nan")], "seed weights must be finite and >= 0"),
                                      ([float("inf"), 1.0], "seed weights must be finite and >= 0"),
                                      ([0.0, 0.0], "the weights of a seed set must have a finite sum > 0"),
                                      ([1e308, 1e308], "the weights of a seed set must have a finite sum > 0")])
def test_bad_weights_are_refused_with_their_text(seeds_plan_check, bad, text):
    with pytest.raises(ValueError):
        sr.weighted_wfix(bad)
    args = ["nan" if w != w else float(w).hex() for w in bad]
    assert _run(seeds_plan_check, "weights", *args).strip() == "refused: " + text


# six nodes, 1 and 4 dangling
ROW_PTR = [0, 2, 2, 3, 5, 5, 6]
# a seed twice in one set; the same seed in two sets; a dangling seed twice; dangling seeds only; a dangling seed first and last
SETS = [[0, 0, 2], [2, 3], [1, 5, 1], [1, 4], [4, 0, 3, 1]]
SETS_ODD = SETS[:3] + [[4]] + SETS[4:]   # an odd number of dangling terms


def _plan(exe, sets, dedup, per):
    words = _run(exe, "plan", int(dedup), per, ",".join(map(str, ROW_PTR)), "/".join(",".join(map(str, s)) for s in sets)).split()
    assert words[-1] == "ok"
    f = dict(w.split("=") for w in words[:-1])
    src = [] if f["slot_src"] == "-" else [int(x) for x in f["slot_src"].split(",")]
    ut = [tuple(int(x) for x in b.split(".")) for b in f["UT"].split(",")] if f["UT"] else []
    return int(f["nl"]), int(f["nd"]), int(f["distinct"]), src, ut


@pytest.mark.parametrize("dedup", [True, False])
def test_slots_by_first_appearance(seeds_plan_check, dedup):
    dangling = {v for v in range(6) if ROW_PTR[v + 1] == ROW_PTR[v]}
    assert dangling == {1, 4}
    for sets in (SETS, SETS_ODD):
        listed = [s for g in sets for s in g]
        live = [s for s in listed if s not in dangling]
        nl, nd, distinct, src, _ = _plan(seeds_plan_check, sets, dedup, 0)
        assert src == (list(dict.fromkeys(live)) if dedup else live) and nl == len(src)
        assert nd == len(listed) - len(live) and distinct == len(set(listed))
    assert _plan(seeds_plan_check, [[1, 4], [4]], dedup, 0)[:4] == (0, 3, 2, [])   # no seed runs at all


def test_batches_and_packs_at_every_parity(seeds_plan_check):
    """per = 1, 2, 3, nl, with and without dedup: the program decodes every batch's list through the view; here, that the
    cases reach both roundings of U + 2 T + 1 halves to words, and an odd and an even number of dangling triples (set[] then
    starts in the middle of a word or node[] does)"""
    parities, nds = set(), set()
    for sets in (SETS, SETS_ODD):
        for dedup in (True, False):
            for per in (1, 2, 3, 0):
                nl, nd, _, _, ut = _plan(seeds_plan_check, sets, dedup, per)
                step = per or nl
                assert len(ut) == (nl + step - 1) // step and sum(u for u, _ in ut) == sum(len(g) for g in sets) - nd
                assert all(1 <= t <= min(u, len(sets)) for u, t in ut)
                parities |= {(u & 1, t & 1) for u, t in ut}
                nds.add(nd & 1)
    assert parities == {(0, 0), (0, 1), (1, 0), (1, 1)} and nds == {0, 1}


def test_chunk_of_rows(seeds_plan_check):
    assert _run(seeds_plan_check, "chunk").split() == ["cases=48", "ok"]


def test_combine_grid(seeds_plan_check):
    assert _run(seeds_plan_check, "grid").split() == ["cases=6", "tile=512", "ok"]
