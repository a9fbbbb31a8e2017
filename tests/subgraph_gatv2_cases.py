"""The table of edge cases of EDGE GATV2 and EDGE GATV2, BACKWARD on the held subgraph, shared by
tests/test_subgraph_gatv2_cases_cpu.py -- which proves from the library's own planning functions and from the constants in the
kernels' headers that the table reaches every lane group of the score step (d) and of the dy step (dv), every vector width and
the tail of the product step for every element type, the staging bound of the forward kernels and every count of column slots of
the backward pass -- and by tests/test_subgraph_gatv2_edges_gpu.py, which runs every row against the numpy twins.  A row that
loses a branch fails on the CPU.

The constants below mirror fora_amd/csrc/fora_subgraph_gatv2.h and fora_subgraph_gatv2_bwd.h; the CPU test reads them out of the
headers' text and holds the two equal."""
from collections import namedtuple

from subgraph_fused_cases import BF16, E4M3, E5M2, ELT_BYTES, F16, F32, TAIL, WIDTHS, Place

GV2_STAGE = 512     # elements of the group's row, and of att, that a wave of the forward kernels stages: hc * d at most
GV2_COLS = 8        # columns a lane of the backward pass owns in one pass over the entries
GV2_FLIGHT = 4      # entries whose gathered rows are in flight
GV2_TILE = 256      # FORA_GATV2_DATT_TILE
SGA_HEADS = 4       # heads of a chunk

DENSE = Place(None, 0)
KINDS = (F32, BF16, F16, E4M3, E5M2)
# kinds: of (xl, xr, att, v, g).  place: of v and g; att_place: of att; xl and xr are dense.  shorts: the values of "attn_short"
# the row runs under
Case = namedtuple("Case", "name heads d dv kinds place att_place shorts slope")

SLOPE = 0.2
LANE_DS = (1, 2, 3, 5, 16, 17, 33, 64, 65, 128, 130)                    # lg = 0 .. 6 of the score step, and a second pass of the lanes
LANE_DVS = (1, 2, 3, 16, 17, 33, 64, 130)                               # of the dy step
STAGING = ((4, 128), (4, 129), (1, 513), (3, 171))                      # hc * d = 512 staged; 516, 513 and 3 * 171 = 513 in place
SLOTS = ((4, 16), (1, 65), (2, 128), (4, 80), (3, 128), (2, 224), (2, 256))   # hc * d = 64, 65, 256 .. 512: nj = 1, 2, 4 .. 8
SLOPES = (0.0, 1.0, -0.5, 3.0)
# the types of (xl, xr, att) beside a narrow v and g: f16 and e5m2 as each of the three, bf16 and e4m3 as att
SMALL = {F32: (F32, F32, F32), BF16: (F32, F32, BF16), F16: (F16, E5M2, F16), E4M3: (F32, F32, E4M3), E5M2: (E5M2, F16, E5M2)}


def _rows():
    rows, f32, both = [], (F32,) * 5, (256, 0)
    row = lambda name, heads, d, dv, kinds=f32, place=DENSE, att_place=DENSE, shorts=both, slope=SLOPE: rows.append(
        Case(name, heads, d, dv, kinds, place, att_place, shorts, slope))
    for d in LANE_DS:
        row(f"lanes-d{d}", 2, d, 8)
    for heads, d in STAGING:
        row(f"stage-h{heads}-d{d}", heads, d, 8)
    for heads, d in SLOTS:
        row(f"slots-h{heads}-d{d}", heads, d, 8)
    for dv in LANE_DVS:
        row(f"lanes-dv{dv}", 2, 3, dv)
    # ---- vector widths of the product step: per type of v and g the widest V, the middle one, V = 1 at an odd pitch, and the tail
    # (the long path once per narrow type)
    for kind in KINDS:
        wide, mid, _ = WIDTHS[ELT_BYTES[kind]]
        tail_dv, tail_pitch = TAIL[ELT_BYTES[kind]]
        name = kind or "f32"
        for what, heads, dv, place in (("wide", 2, wide, DENSE), ("mid", 2, 3 * mid, DENSE), ("view", 2, wide, Place(2 * wide + 5, 3)),
                                       ("tail", 1, tail_dv, Place(tail_pitch, 0))):
            row(f"{name}-{what}", heads, 8, dv, SMALL[kind] + (kind, kind), place, shorts=both if kind is F32 or what == "wide" else (256,))
    for heads in (4, 8, 9):                                             # whole chunks only, and three chunks with a ragged last one
        row(f"heads{heads}", heads, 8, 8)
    for slope in SLOPES:
        row(f"slope{slope:g}", 3, 8, 8, slope=slope)
    # ---- att as the view wide[:, off:off + d] of a wider array: ldatt > d
    row("attview-f32", 3, 5, 8, att_place=Place(11, 3))
    row("attview-e4m3", 2, 8, 8, kinds=(F32, F32, E4M3, F32, F32), att_place=Place(13, 2))
    return tuple(rows)


CASES = _rows()


def operands(case):
    """((name, kind, rows or None for the held columns, columns a head, heads side by side, pitch in elements, first column of the
    view), ...) of the five operands of a row: att is [heads, d], the others [nc, heads * width]"""
    out = []
    for name, kind in zip(("xl", "xr", "att", "v", "g"), case.kinds):
        w = case.dv if name in ("v", "g") else case.d
        rows, side = (case.heads, 1) if name == "att" else (None, case.heads)
        place = case.place if name in ("v", "g") else case.att_place if name == "att" else DENSE
        out.append((name, kind, rows, w, side, place.pitch or side * w, place.off))
    return tuple(out)


def chunks(case):
    """hc * d of every chunk of up to SGA_HEADS heads of a row, with its hc"""
    return [(min(SGA_HEADS, case.heads - h0) * case.d, min(SGA_HEADS, case.heads - h0)) for h0 in range(0, case.heads, SGA_HEADS)]


def column_slots(wc):
    """nj of every pass of the backward pass over a chunk of wc columns: min(GV2_COLS, ceil((wc - c0) / 64))"""
    return [min(GV2_COLS, (wc - c0 + 63) // 64) for c0 in range(0, wc, 64 * GV2_COLS)]
