"""The case table of tests/subgraph_fused_cases.py on the CPU: what the library's own planning functions decide for every row
(tests/subgraph_fused_cases_check.cpp: attn_vec_width, prop_group_lg and prop_widths_bytes of fora_amd/csrc, a stand-alone program
built here), so that the matrix of tests/test_subgraph_fused_edges_gpu.py provably reaches every vector width of every element type,
the tail of the product step, every lane group of the score step and the head passes of k_sub_gat_across.  Whoever edits a shape and
loses a branch fails here."""
import os
import subprocess

import numpy as np
import pytest

import subgraph_fused_cases as fc
import subgraph_prop_ref as sr
import subgraph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fused_cases") / "subgraph_fused_cases_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "subgraph_fused_cases_check.cpp")], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = [[int(t) for t in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def test_the_table_names_the_librarys_widths_and_unique_rows(ask):
    for elt, widths in fc.WIDTHS.items():
        assert tuple(ask([f"widths {elt}"])[0]) == widths
    for rows in (fc.ATTN, fc.GAT):
        assert len({c.name for c in rows}) == len(rows)
    assert all(set(c.shorts) <= {256, 0} and c.shorts for c in fc.CASES) and all(c.d == 1 for c in fc.GAT)


def test_every_width_of_every_type_and_the_tail_are_reached(ask):
    asked = [(c, op) for c in fc.CASES for op in fc.operands(c) if op[0] in ("v", "g")]
    answers = ask([f"vec {off} {ld} {w} {c.heads} {fc.ELT_BYTES[kind]}" for c, (_, kind, w, ld, off) in asked])
    reached, tails, long_path = set(), set(), set()
    for (c, (name, kind, w, ld, off)), (v_in_place, v_uploaded) in zip(asked, answers):
        assert v_in_place == v_uploaded, (c.name, name)          # the row means the same for a host and a device operand
        assert off + c.heads * w <= ld
        reached.add((c.call, name, kind, v_uploaded))
        if c.heads == 1 and v_uploaded > 1 and w % v_uploaded:
            tails.add((c.call, name, kind))
        if 0 in c.shorts:
            long_path.add((c.call, kind))
    kinds = (fc.F32, fc.BF16, fc.F16, fc.E4M3, fc.E5M2)
    for call in ("attn", "gat"):
        for name in ("v", "g"):
            for kind in kinds:
                for V in fc.WIDTHS[fc.ELT_BYTES[kind]]:
                    assert (call, name, kind, V) in reached, (call, name, kind, V)
                assert (call, name, kind) in tails, (call, name, kind)
        assert {(call, kind) for kind in kinds} <= long_path
    # f16 and e5m2 as q, k, el and er, each at least once
    for call, names in (("attn", ("q", "k")), ("gat", ("el", "er"))):
        small = {(name, kind) for c in fc.CASES if c.call == call for name, kind, *_ in fc.operands(c)}
        assert {(n, k) for n in names for k in (fc.F16, fc.E5M2)} <= small


def test_every_lane_group_of_the_score_step_is_reached(ask):
    lg = lambda values: {v: ask([f"lg {v}"])[0][0] for v in sorted(set(values))}
    every = set(range(7))
    d_attn, dv_attn, dv_gat = lg(c.d for c in fc.ATTN), lg(c.dv for c in fc.ATTN), lg(c.dv for c in fc.GAT)
    for name, table in (("d of attention", d_attn), ("dv of attention", dv_attn), ("dv of gat", dv_gat)):
        assert set(table.values()) == every, (name, table)
        assert max(table) > 64, name                              # a second pass of the 64 lanes
        assert table[1] == 0 and table[2] == 1, name              # G = 1 and G = 2: no exchange, one


def test_the_head_counts_reach_the_passes_of_the_across_kernel():
    row_ptr, col, U = sr.crafted_graph()
    sub_ptr, sub_col = subgraph_ref.induced(row_ptr, col, U)[:2]
    sides = {"rows": np.diff(sub_ptr), "columns": np.bincount(sub_col, minlength=sr.CRAFTED_NC)}
    heads = {c.heads for c in fc.GAT}
    assert {4, 8, 9, 67} <= heads and {4, 8, 9} <= {c.heads for c in fc.ATTN}
    for name, lens in sides.items():
        for length in (255, 256):                                 # a full pass followed by another, then a ragged one
            assert length in lens and fc.head_passes(length, 9) == [4, 4, 1], (name, length)
        small = lens[(lens > 0) & (lens <= 15)]
        assert small.size > 600, name                             # the filler nodes
        for length in np.unique(small).tolist():                  # the cap of 64 heads a pass, then the rest
            assert fc.head_passes(length, 67) == [64, 3], (name, length)
        assert (lens == 0).any()                                  # the empty group's loop takes a second step with 67 heads
    assert fc.head_passes(63, 8) == [8] and fc.head_passes(205, 5) == [5] and fc.head_passes(206, 5) == [4, 1] == fc.head_passes(257, 5)
