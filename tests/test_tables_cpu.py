"""The graph's derived tables (fora_amd/csrc/fora_tables.h) built and checked on the CPU: tests/tables_check.cpp restates
how the kernels read each table and runs, under the address and undefined-behaviour sanitizers, on the smallest graphs
that reach every branch of the builders.  The sanitized code is that stand-alone program and nothing else."""
import os
import subprocess
import time

import numpy as np
import pytest

from fora_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def tables_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tables") / "tables_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "tables_check.cpp")], check=True)
    return exe


def _write(path, row_ptr, col):
    row_ptr = np.ascontiguousarray(row_ptr, dtype="<i8")
    col = np.ascontiguousarray(col, dtype="<i4")
    with open(path, "wb") as f:
        f.write(np.array([row_ptr.size - 1, col.size], dtype="<i8").tobytes())
        f.write(row_ptr.tobytes())
        f.write(col.tobytes())
    return str(path)


def _run(exe, path, shift=13, pbins=0, force=0, max_members=32, team_hubs=0, push_hubs=0, dg_hubs=0, tables=()):
    """Facts of a passing run as a dict; a failed property fails the test with the program's line."""
    r = subprocess.run([exe, path, *map(str, (shift, pbins, force, max_members, team_hubs, push_hubs, dg_hubs)), *tables],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[-1] == "ok"
    return {k: int(v) for k, v in (w.split("=") for w in words[:-1])}


def _rows_from_degrees(n, deg):
    """Node i with out-degree deg[i], targets (i + 1 + k) % n."""
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=row_ptr[1:])
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    k = np.arange(row_ptr[-1], dtype=np.int64) - row_ptr[src]
    return row_ptr, ((src + 1 + k) % n).astype(np.int32)


def _tiny(dangling, rows):
    """The tiny preset; rows "shuffled": every row in a random order (the generator's rows ascend), "sorted": as generated."""
    n, m, seed = synth.PRESETS["tiny"]
    row_ptr, col = synth.csr_from_edges(n, *synth.rmat_graph(n, m, seed, dangling))
    if rows == "shuffled":
        rng = np.random.Generator(np.random.PCG64(7))
        col = col[np.lexsort((rng.random(col.size), np.repeat(np.arange(n), np.diff(row_ptr))))]
    return n, row_ptr, col


# every (team force, team hubs) pair and every (push hubs, shift) pair once
TINY_RUNS = [(0, 0, 0, 13), (0, 64, 64, 6), (2, 0, 5000, 13), (2, 64, 0, 6), (4, 0, 64, 13), (4, 64, 5000, 6)]


@pytest.mark.parametrize("dangling", ["rmat", "none"])
def test_tiny(tables_check, tmp_path, dangling):
    n, row_ptr, col = _tiny(dangling, "shuffled")
    path = _write(tmp_path / "g.csr", row_ptr, col)
    for force, team_hubs, push_hubs, shift in TINY_RUNS:
        f = _run(tables_check, path, shift=shift, pbins=11 if shift == 6 else 0, force=force, team_hubs=team_hubs, push_hubs=push_hubs)
        assert f["dg_have"] == 1 and f["team_T"] == max(1, force) and f["team_H"] == team_hubs
        assert (f["dangling"] > 0) == (dangling == "rmat")
        assert (f["dg_zero_first"] < f["dg_np"]) == (dangling == "rmat")  # a zero class, or zero_first == np
        assert f.get("hubs_H", 0) == min(push_hubs, n)
        assert f["npass"] == (3 if shift == 6 else 1) and f.get("split_sorted", 0) == 0


def test_tiny_sorted_rows_and_member_limit(tables_check, tmp_path):
    n, row_ptr, col = _tiny("none", "sorted")
    path = _write(tmp_path / "g.csr", row_ptr, col)
    f = _run(tables_check, path, shift=6, pbins=11, force=4, max_members=2)  # three passes without a sorted copy; no T in 4 .. 2
    assert f["npass"] == 3 and f["split_sorted"] == 1 and f["team_T"] == 0


def test_all_hubs(tables_check, tmp_path):
    """n <= 256: every node a hub record, no classes, T four zero bytes.  A ring with a few chords, node 7 without out-edges."""
    n = 200
    rows = [[(i + 1) % n] + ([(i * 7 + 3) % n, (i + 50) % n] if i % 9 == 0 else []) for i in range(n)]
    rows[7] = []
    row_ptr = np.cumsum([0] + [len(r) for r in rows])
    f = _run(tables_check, _write(tmp_path / "g.csr", row_ptr, [t for r in rows for t in r]), team_hubs=64, push_hubs=64)
    assert f["dg_have"] == 1 and f["dg_H"] == n and f["dg_ncls"] == 0 and f["dangling"] == 1 and f["dg_zero_first"] == n - 1


def test_hub_ladder(tables_check, tmp_path):
    """600 distinct out-degrees: 256 and 512 hubs leave more than 255 of them, 1024 do not.  dg_hubs 2048 is clipped to n: at
    n = 1200 the 1200 hub records take 1201 * 8 + 1200 * 16 + 4 = 28 812 bytes of LDS, over the 28 KiB cap -- no copy; at
    n = 1100 (550 distinct out-degrees, the same ladder) they fit."""
    for n, all_hubs_fit in ((1200, False), (1100, True)):
        path = _write(tmp_path / f"g{n}.csr", *_rows_from_degrees(n, np.arange(n) % (n // 2)))
        assert _run(tables_check, path, team_hubs=64, push_hubs=64)["dg_H"] == 1024
        f = _run(tables_check, path, dg_hubs=2048)
        assert f["dg_have"] == all_hubs_fit and (not all_hubs_fit or (f["dg_H"] == n and f["dg_ncls"] == 0))


def test_no_walk_copy(tables_check, tmp_path):
    """4352 distinct out-degrees: 4096 hubs still leave 256 classes -- no copy, and no time spent on one (the run reads 9.5 M
    edges and looks at five hub counts: a tenth of a second)."""
    n = 4352
    path = _write(tmp_path / "g.csr", *_rows_from_degrees(n, np.arange(n)))
    t0 = time.perf_counter()
    f = _run(tables_check, path, tables=["dg"])
    took = time.perf_counter() - t0
    print(f"walk copy of the 4352-node graph: {took:.3f} s")
    assert f["dg_have"] == 0 and took < 1.0


def test_quads_and_last_words(tables_check, tmp_path):
    """Out-degrees 0, 1, 4, 5 with a duplicate edge: quads 0 + 1 + 1 + 2, and packed lists of a few words."""
    rows = [[], [2], [0, 1, 3, 3], [0, 1, 2, 0, 1]]
    row_ptr = np.cumsum([0] + [len(r) for r in rows])
    f = _run(tables_check, _write(tmp_path / "g.csr", row_ptr, [t for r in rows for t in r]), shift=1, pbins=1, team_hubs=2, push_hubs=2)
    assert f["quads"] == 4 and f["dg_H"] == 4 and f["npass"] == 2 and f["split_sorted"] == 0
