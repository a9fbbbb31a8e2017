"""The line-aligned flush of k_walk_dg's result stages (fora_amd/csrc/fora_flush_plan.h: head, send, cap, the bins' words
and the slots of the rebuilt stage) on the CPU: tests/flush_plan_check.cpp plays the waves of a workgroup over many flushes
and a closing one, for lines of 8 and 16 results, 1 to 128 bins, several stage lengths and caps, aligned and unaligned
starting fills, under the address and undefined-behaviour sanitizers.  The sanitized code is that stand-alone program and
nothing else."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def flush_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flush") / "flush_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "flush_plan_check.cpp")], check=True)
    return exe


def test_every_result_leaves_once_in_whole_lines(flush_check):
    r = subprocess.run([flush_check, "6"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    print(r.stdout.strip())
    assert r.stdout.split()[-1] == "ok", r.stdout
    # both kinds of flush ran: aligned ones and the progress rule's full ones
    stats = dict(w.split("=") for w in r.stdout.split()[:-1])
    assert int(stats["full"]) > 0 and int(stats["flushes"]) > 10 * int(stats["runs"])


def test_flush_arms_register_file():
    """The arms of the option "walk_flush_align" in the shipped library (tools/isa_audit.py on its code-object notes): the
    default k_walk_dg and the two other arms of every instantiation, at most 64 VGPRs, no VGPR spill, no scratch, and the
    same static LDS in all three -- the carried results live in the stage, so a CU still takes three workgroups."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    from fora_amd import build as b
    rows = {r["kernel"]: r for r in isa_audit.audit(b.build_hip())}
    arms = sorted(k for k in rows if k.startswith("k_flush_arm_walk_dg<"))
    assert len(arms) == 16 and {k.split("<")[1].split(",")[0] for k in arms} == {"0", "16"}, arms   # the default, 8, is k_walk_dg itself
    for k in arms:
        base = rows["k_walk_dg<" + k.split(",", 1)[1]]
        for r in (rows[k], base):
            assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0 and r["scratch"] == 0 and r.get("agpr", 0) == 0, r
            assert 0 < r["vgpr"] <= 64, (r["kernel"], r["vgpr"])
        assert rows[k]["lds_static"] == base["lds_static"], (k, rows[k]["lds_static"], base["lds_static"])
