"""The ticket -> tile mapping of k_walk_dg's hand-out (fora_amd/csrc/fora_consts.h: dg_ticket_tile) on the CPU:
tests/walk_dg_tickets_check.cpp plays the hand-out of every workgroup of a slot, waves asking in any order, for every
item count from 0 to 5000 and a few (workgroups, waves, tile) shapes, one workgroup per slot among them, under the
address and undefined-behaviour sanitizers.  The sanitized code is that stand-alone program and nothing else."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tickets_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tickets") / "walk_dg_tickets_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "walk_dg_tickets_check.cpp")], check=True)
    return exe


def test_tickets_cover_every_tile_once(tickets_check):
    r = subprocess.run([tickets_check, "5000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    assert r.stdout.split()[-1] == "ok", r.stdout
