// fora_prop_plan.h -- the host side of PROPAGATE (fora_hip_sparse_propagate; include/fora_hip.h): what the caller's
// row_ptr says about the work.  A row is cut every PROP_SEG entries from its first entry; the segments of all rows, in row
// order, are the work list of the gather kernel; a call runs them in chunks of at most `prop_segs` segments, the partial
// sums of one chunk live at a time.  Integer code, no HIP, no context -- fora_hip.hip owns buffers and launches,
// tests/prop_plan_check.cpp restates the partition by brute force without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace fora {

constexpr uint32_t PROP_SEG = 256; // FORA_PROP_SEG of include/fora_hip.h (fora_hip.hip holds the two equal)

// One segment: entries [first, first + len) of the held result, 1 <= len <= PROP_SEG, of row `row`; its partial sum goes
// to slot `slot` of the chunk's partial-sum buffer (the segment's position inside its chunk).
struct PropSeg { int64_t first; uint32_t len, slot; int32_t row; uint32_t pad_; };
// What the combine kernel does for one row in one chunk: add the partial sums of slots [slot0, slot0 + nseg) in order.
// PROP_FIRST: the row's segment 0 is among them (the sum starts there; otherwise from the carry the chunk before left).
// PROP_LAST: so is its last one (the row is finished and written; otherwise the sum is left as the carry).  A chunk cuts
// the segment list anywhere, so at most its first record lacks PROP_FIRST and at most its last one lacks PROP_LAST.
// An empty row has nseg == 0 and both flags: it is written as +0.0 by the chunk that is open when it comes.
enum : uint32_t { PROP_FIRST = 1, PROP_LAST = 2 };
struct PropRowRec { int32_t row; uint32_t slot0, nseg, flags; };
struct PropChunk { uint64_t seg0 = 0, nseg = 0, rec0 = 0, nrec = 0; };

struct PropPlan {
    std::vector<PropSeg> segs;      // all segments of the call, in row order
    std::vector<PropRowRec> recs;   // all row records, chunk by chunk
    std::vector<PropChunk> chunks;  // empty only when nq == 0
    uint64_t entries = 0, max_row = 0;
};

// the caller's row_ptr against the held result: starts at 0, never decreases, ends at the held entries
inline bool prop_row_ptr_ok(const int64_t *row_ptr, int nq, uint64_t held_entries) {
    if (!row_ptr || nq < 0 || row_ptr[0] != 0) return false;
    for (int i = 0; i < nq; i++)
        if (row_ptr[i + 1] < row_ptr[i]) return false;
    return (uint64_t)row_ptr[nq] == held_entries;
}

inline uint64_t prop_segments(const int64_t *row_ptr, int nq) {
    uint64_t s = 0;
    for (int i = 0; i < nq; i++) s += ((uint64_t)(row_ptr[i + 1] - row_ptr[i]) + PROP_SEG - 1) / PROP_SEG;
    return s;
}

// the option "prop_segs" as a number of segments per chunk: 0 (or less) means by free memory -- a quarter of it in partial
// sums (d doubles and one word sum per segment) at most; never more than the call has, never less than 1
inline uint64_t prop_chunk_segs(int64_t option, uint64_t segments, uint64_t free_bytes, int d) {
    const uint64_t per = option > 0 ? (uint64_t)option : std::max<uint64_t>(1, free_bytes / 4 / ((uint64_t)d * 8 + 8));
    return std::min<uint64_t>({per, std::max<uint64_t>(segments, 1), 1ull << 30});
}

// prop_segs: segments per chunk, at least 1 (prop_chunk_segs has resolved the option to a number).  row_ptr has passed
// prop_row_ptr_ok.  A chunk is closed only when a further segment no longer fits, so empty rows never open one of their
// own: chunks == max(1, ceil(segments / prop_segs)) for nq > 0.
// keep(i, len): the rows that take part -- a row it refuses gets no segment and no record, as if the list were made for the
// others alone (ATTENTION plans its longer rows this way, fora_attn_plan.h); entries and max_row are of the rows kept.
template <typename Keep>
inline PropPlan prop_plan_if(const int64_t *row_ptr, int nq, uint64_t prop_segs, Keep keep) {
    PropPlan p;
    prop_segs = std::max<uint64_t>(prop_segs, 1);
    if (nq <= 0) return p;
    p.chunks.push_back(PropChunk{});
    for (int i = 0; i < nq; i++) {
        const uint64_t len = (uint64_t)(row_ptr[i + 1] - row_ptr[i]);
        if (!keep(i, len)) continue;
        p.entries += len;
        p.max_row = std::max(p.max_row, len);
        if (!len) {
            p.recs.push_back(PropRowRec{i, 0, 0, PROP_FIRST | PROP_LAST});
            p.chunks.back().nrec++;
            continue;
        }
        const uint64_t ns = (len + PROP_SEG - 1) / PROP_SEG;
        for (uint64_t s = 0; s < ns;) {
            if (p.chunks.back().nseg == prop_segs) { // full: the next one starts here
                const PropChunk &b = p.chunks.back();
                p.chunks.push_back(PropChunk{b.seg0 + b.nseg, 0, b.rec0 + b.nrec, 0});
            }
            PropChunk &ch = p.chunks.back();
            const uint64_t take = std::min(ns - s, prop_segs - ch.nseg);
            p.recs.push_back(PropRowRec{i, (uint32_t)ch.nseg, (uint32_t)take, (s == 0 ? PROP_FIRST : 0u) | (s + take == ns ? PROP_LAST : 0u)});
            ch.nrec++;
            for (uint64_t k = 0; k < take; k++, s++) {
                const uint64_t at = s * PROP_SEG;
                p.segs.push_back(PropSeg{row_ptr[i] + (int64_t)at, (uint32_t)std::min<uint64_t>(PROP_SEG, len - at), (uint32_t)(ch.nseg + k), i, 0});
            }
            ch.nseg += take;
        }
    }
    return p;
}
inline PropPlan prop_plan(const int64_t *row_ptr, int nq, uint64_t prop_segs) {
    return prop_plan_if(row_ptr, nq, prop_segs, [](int, uint64_t) { return true; });
}

// ---- how the gather kernel's lanes map to columns (prop_geom): a lane takes V adjacent columns of one feature row, a
// group of G lanes (a power of two, 1 .. 64) a tile of G * V columns, so that a group's load is contiguous bytes of the
// row; a wave holds 64 / G groups, each with a segment of its own -- with d = 1 a wave sums 64 segments, not one on one
// lane.  V: the widest of `widths` (descending, ending in 1) that base and pitch alignment allow and d fills.
struct PropGeom { uint32_t V = 1, G = 64, tiles = 1, segs_per_wave = 1; };
inline PropGeom prop_geom(uint64_t feat_addr, int64_t ldf, int d, uint32_t elt_bytes, const uint32_t *widths, int nwidths) {
    PropGeom g;
    for (int i = 0; i < nwidths; i++) {
        const uint32_t V = widths[i];
        if (V == 1 || (V <= (uint32_t)d && feat_addr % ((uint64_t)V * elt_bytes) == 0 && ldf % (int64_t)V == 0)) { g.V = V; break; }
    }
    const uint32_t lanes = ((uint32_t)d + g.V - 1) / g.V; // lanes that one row's d columns take
    g.G = 1;
    while (g.G < 64 && g.G < lanes) g.G *= 2;
    g.tiles = (lanes + g.G - 1) / g.G;
    g.segs_per_wave = 64 / g.G;
    return g;
}
// the `widths` of an element type, PROP_NWIDTHS of them: 16 bytes a lane at most
constexpr int PROP_NWIDTHS = 3;
inline const uint32_t *prop_widths(bool bf16) {
    static const uint32_t f32[PROP_NWIDTHS] = {4, 2, 1}, b16[PROP_NWIDTHS] = {8, 4, 1};
    return bf16 ? b16 : f32;
}
// the same by element size: the two tables above for 4 and 2 bytes (f16 lies as bf16 does), and for the one-byte types
// (FP8) 16 columns -- four words, the widest load -- then one word, then one byte
inline const uint32_t *prop_widths_bytes(uint32_t elt_bytes) {
    static const uint32_t b8[PROP_NWIDTHS] = {16, 4, 1};
    return elt_bytes == 1 ? b8 : prop_widths(elt_bytes == 2);
}
// the group exponent: the smallest lg <= 6 with 2^lg >= d -- the lanes that share a d-column dot product, at most a wave
inline uint32_t prop_group_lg(uint32_t d) {
    uint32_t lg = 0;
    while (lg < 6 && (1u << lg) < d) lg++;
    return lg;
}
// the bytes of a caller's operand from its first element to its last: a matrix of `rows` rows of `width` elements at pitch
// ld >= width (nothing follows the last row), a vector of `count` elements; no rows are no bytes
inline uint64_t prop_matrix_bytes(uint64_t rows, uint64_t ld, uint64_t width, uint32_t elt_bytes) { return rows ? ((rows - 1) * ld + width) * elt_bytes : 0; }
inline uint64_t prop_vector_bytes(uint64_t count, uint32_t elt_bytes) { return count * elt_bytes; }
// the segments of the rows longer than cap: the ones ATTENTION leaves to the three steps' kernels (fora_attn_plan.h)
inline uint64_t prop_long_segments(const int64_t *row_ptr, int nq, uint32_t cap) {
    uint64_t s = 0;
    for (int i = 0; i < nq; i++) {
        const uint64_t len = (uint64_t)(row_ptr[i + 1] - row_ptr[i]);
        if (len > cap) s += (len + PROP_SEG - 1) / PROP_SEG;
    }
    return s;
}

} // namespace fora
