"""The case table of tests/subgraph_gatv2_cases.py on the CPU: what the library's own planning functions decide for every row
(tests/subgraph_fused_cases_check.cpp, a stand-alone program built here) and what the constants of the kernels' headers make of
its shapes, so that the matrix of tests/test_subgraph_gatv2_edges_gpu.py provably reaches every lane group of the score step and
of the dy step, every vector width of every element type of v and g with the tail, the long path for every type, the staging
bound of the forward kernels from both sides and every count of column slots of the backward pass.  Whoever edits a shape and
loses a branch fails here."""
import os
import re

import subgraph_gatv2_cases as gc
from test_subgraph_fused_cases_cpu import ask  # noqa: F401  (the module-scoped fixture: the program built, one answer a line)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_table_mirrors_the_headers_constants_and_has_unique_rows(ask):
    text = ""
    for name in ("fora_subgraph_attn.h", "fora_subgraph_gatv2.h", "fora_subgraph_gatv2_bwd.h"):   # (device code: not for g++)
        with open(os.path.join(ROOT, "fora_amd", "csrc", name)) as f:
            text += f.read()
    for name in ("GV2_STAGE", "GV2_COLS", "GV2_FLIGHT", "GV2_TILE", "SGA_HEADS"):
        found = re.findall(r"constexpr\s+(?:uint32_t|int)\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert found == [str(getattr(gc, name))], (name, found)
    assert (gc.GV2_STAGE, gc.GV2_COLS, gc.GV2_FLIGHT, gc.GV2_TILE) == (512, 8, 4, 256) and 64 * gc.GV2_COLS == gc.GV2_STAGE
    for elt, widths in gc.WIDTHS.items():
        assert tuple(ask([f"widths {elt}"])[0]) == widths
    assert len({c.name for c in gc.CASES}) == len(gc.CASES)
    assert all(set(c.shorts) <= {256, 0} and c.shorts for c in gc.CASES)


def test_every_lane_group_of_the_score_step_and_of_the_dy_step_is_reached(ask):
    lg = lambda values: {v: ask([f"lg {v}"])[0][0] for v in sorted(set(values))}
    for name, table in (("d", lg(c.d for c in gc.CASES)), ("dv", lg(c.dv for c in gc.CASES))):
        assert set(table.values()) == set(range(7)), (name, table)
        assert max(table) > 64, name                                  # a second pass of the 64 lanes
        assert table[1] == 0 and table[2] == 1, name                  # G = 1 and G = 2: no exchange, one
    assert {c.d for c in gc.CASES} >= {64, 65, 128} and any(c.d > gc.GV2_STAGE for c in gc.CASES)


def test_every_width_of_every_type_of_v_and_g_and_the_tail_are_reached(ask):
    asked = [(c, op) for c in gc.CASES for op in gc.operands(c) if op[0] in ("v", "g")]
    answers = ask([f"vec {off} {ld} {w} {c.heads} {gc.ELT_BYTES[kind]}" for c, (_, kind, _, w, _, ld, off) in asked])
    reached, tails, long_path = set(), set(), set()
    for (c, (name, kind, _, w, side, ld, off)), (v_in_place, v_uploaded) in zip(asked, answers):
        assert v_in_place == v_uploaded, (c.name, name)               # the row means the same for a host and a device operand
        assert side == c.heads and off + side * w <= ld
        reached.add((name, kind, v_uploaded))
        if c.heads == 1 and v_uploaded > 1 and w % v_uploaded:
            tails.add((name, kind))
        if 0 in c.shorts:
            long_path.add(kind)
    for name in ("v", "g"):
        for kind in gc.KINDS:
            for V in gc.WIDTHS[gc.ELT_BYTES[kind]]:
                assert (name, kind, V) in reached, (name, kind, V)
            assert (name, kind) in tails, (name, kind)
    assert set(gc.KINDS) <= long_path
    # f16 and e5m2 as xl, xr and att; bf16 and e4m3 as att; att as a view of f32 and of a 1-byte kind
    small = {(name, kind) for c in gc.CASES for name, kind, *_ in gc.operands(c)}
    assert {(n, k) for n in ("xl", "xr", "att") for k in (gc.F16, gc.E5M2)} | {("att", gc.BF16), ("att", gc.E4M3)} <= small
    views = {kind for c in gc.CASES for name, kind, _, w, _, ld, off in gc.operands(c) if name == "att" and ld > w and off > 0 and c.heads > 1}
    assert gc.F32 in views and any(gc.ELT_BYTES[k] == 1 for k in views)


def test_the_staging_bound_and_every_count_of_column_slots_are_reached():
    chunks = [(wc, hc, c) for c in gc.CASES for wc, hc in gc.chunks(c)]
    assert {gc.column_slots(wc)[0] for wc, _, _ in chunks} == set(range(1, gc.GV2_COLS + 1))
    assert any(wc == gc.GV2_STAGE for wc, _, _ in chunks)             # the last staged chunk; backward, no second pass
    assert all(len(gc.column_slots(wc)) == 1 for wc, _, _ in chunks if wc <= gc.GV2_STAGE)
    assert {hc for wc, hc, _ in chunks if wc > gc.GV2_STAGE} == {1, 3, 4}   # in place: no division, one by 3, one by 4
    assert any(gc.column_slots(wc) == [8, 1] for wc, _, _ in chunks)  # 8 slots, then a second pass of one
    # the single-chunk rows of 64, 65, 256 .. 512 columns; two or more with a head boundary inside a lane's stride
    single = {gc.chunks(c)[0][0]: c for c in gc.CASES if c.name.startswith("slots-")}
    assert sorted(single) == [64, 65, 256, 320, 384, 448, 512] and all(c.heads <= gc.SGA_HEADS for c in single.values())
    assert sum(c.heads > 1 and c.d % 64 != 0 for c in single.values()) >= 2
    assert {4, 8, 9} <= {c.heads for c in gc.CASES if (c.d, c.dv) == (8, 8)}
    assert {c.slope for c in gc.CASES} >= {0.0, 1.0, -0.5, 3.0, gc.SLOPE}
