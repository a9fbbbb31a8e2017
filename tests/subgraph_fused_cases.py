"""The table of edge cases of the four fused calls on the held subgraph (EDGE ATTENTION, EDGE GAT and their backward calls), shared
by tests/test_subgraph_fused_cases_cpu.py -- which proves from the library's own planning functions that the table reaches every
lane group of the score step, every vector width and the tail of the product step and the head passes it is meant to reach -- and by
tests/test_subgraph_fused_edges_gpu.py, which runs every row against the numpy twins.  A row that loses a branch fails on the CPU.

A host operand is uploaded from its first element into a buffer of the library's own, so the kernels see an aligned base whatever
the column a view starts at; an operand on the device is read in place at its own address.  Every row here is chosen so that the
width is the same under both: the CPU test asks the planner about both addresses and holds them equal."""
from collections import namedtuple

import narrow_ref

F32, BF16, F16, E4M3, E5M2 = None, "bf16", narrow_ref.F16, narrow_ref.E4M3, narrow_ref.E5M2     # the kinds as the twins name them
ELT_BYTES = {F32: 4, BF16: 2, F16: 2, E4M3: 1, E5M2: 1}
WIDTHS = {4: (4, 2, 1), 2: (8, 4, 1), 1: (16, 4, 1)}          # prop_widths_bytes of fora_prop_plan.h (the CPU test holds the two equal)
TAIL = {4: (6, 8), 2: (12, 16), 1: (20, 32)}                  # (dv, pitch) of the tail: pitch a multiple of the widest V, dv not
GAT_X_LDS = 1028                                              # doubles of a wave of k_sub_gat_across

# pitch None: dense.  Otherwise the operand is the view wide[:, off:off + width] of an array of `pitch` columns
Place = namedtuple("Place", "pitch off")
DENSE = Place(None, 0)
# call: "attn" or "gat".  kinds: of (q, k, v, g) or (el, er, v, g).  place: of v and g; q, k, el and er are dense.  param: scale or
# slope.  shorts: the values of "attn_short" the row runs under
Case = namedtuple("Case", "name call heads d dv kinds place shorts param")

SCALE, SLOPE = 0.375, 0.2
LANE_SHAPES = ((1, 2), (2, 1), (3, 3), (4, 16), (16, 4), (17, 32), (33, 130), (64, 64), (130, 2))   # (d, dv) of EDGE ATTENTION
LANE_DVS = (1, 2, 3, 16, 17, 33, 64, 130)                                                          # dv of EDGE GAT
SCALES, SLOPES = (-1.75, 0.0, 2.0 ** -20), (0.0, 1.0, -0.5, 3.0)


def _param(call):
    return SCALE if call == "attn" else SLOPE


def _rows():
    rows, f32 = [], (F32,) * 4
    both = (256, 0)
    # ---- lane groups of the score step: G = 1 .. 64 and a second pass, for d (forward) and dv (backward)
    for d, dv in LANE_SHAPES:
        rows.append(Case(f"lanes-d{d}-dv{dv}", "attn", 2, d, dv, f32, DENSE, both, SCALE))
    for dv in LANE_DVS:
        rows.append(Case(f"lanes-dv{dv}", "gat", 2, 1, dv, f32, DENSE, both, SLOPE))
    # ---- vector widths of the product step: per type of v and g the widest V, the middle one, V = 1 at an odd pitch, and the tail
    # (the long path once per narrow type; f16 and e5m2 also as q, k, el and er)
    for kind in (F32, BF16, F16, E4M3, E5M2):
        wide, mid, _ = WIDTHS[ELT_BYTES[kind]]
        tail_dv, tail_pitch = TAIL[ELT_BYTES[kind]]
        small = {F16: (F16, E5M2), E5M2: (E5M2, F16)}.get(kind, (F32, F32))
        name = kind or "f32"
        for call in ("attn", "gat"):
            for what, heads, dv, place in (("wide", 2, wide, DENSE), ("mid", 2, 3 * mid, DENSE), ("view", 2, wide, Place(2 * wide + 5, 3)),
                                           ("tail", 1, tail_dv, Place(tail_pitch, 0))):
                shorts = both if kind is F32 or what == "wide" else (256,)
                rows.append(Case(f"{name}-{what}", call, heads, 8 if call == "attn" else 1, dv, small + (kind, kind), place, shorts, _param(call)))
    # ---- head counts: whole chunks only (4, 8), three chunks with a full pass of k_sub_gat_across followed by another (9), and its
    # cap of 64 heads a pass (67)
    for call in ("attn", "gat"):
        for heads in (4, 8, 9):
            rows.append(Case(f"heads{heads}", call, heads, 8 if call == "attn" else 1, 8, f32, DENSE, both, _param(call)))
    rows.append(Case("heads67", "gat", 67, 1, 1, f32, DENSE, both, SLOPE))
    # ---- scale and slope
    for scale in SCALES:
        rows.append(Case(f"scale{scale:g}", "attn", 3, 8, 8, f32, DENSE, both, scale))
    for slope in SLOPES:
        rows.append(Case(f"slope{slope:g}", "gat", 3, 1, 8, f32, DENSE, both, slope))
    return tuple(rows)


CASES = _rows()
ATTN = tuple(c for c in CASES if c.call == "attn")
GAT = tuple(c for c in CASES if c.call == "gat")


def operands(case):
    """((name, kind, columns a head, pitch in elements, first column of the view), ...) of the four operands of a row"""
    names = ("q", "k", "v", "g") if case.call == "attn" else ("el", "er", "v", "g")
    out = []
    for name, kind in zip(names, case.kinds):
        w = case.dv if name in ("v", "g") else case.d
        place = case.place if name in ("v", "g") else DENSE
        out.append((name, kind, w, place.pitch or case.heads * w, place.off))
    return tuple(out)


def head_passes(length, heads):
    """the heads of every pass of k_sub_gat_across over a group of `length` edges"""
    per = min(64, GAT_X_LDS // (length | 1))
    return [min(per, heads - hb) for hb in range(0, heads, per)]
