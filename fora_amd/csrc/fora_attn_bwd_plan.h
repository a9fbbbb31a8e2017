// fora_attn_bwd_plan.h -- the host side of ATTENTION, BACKWARD (fora_hip_sparse_attention_bwd; include/fora_hip.h).  The rows
// are split by the option "attn_short" exactly as the forward call splits them (attn_plan, fora_attn_plan.h); this file holds
// the same split of the COLUMNS of the transposition, from its col_ptr:
//   shrt   one PropSeg per non-empty column of at most `attn_short` entries -- first (in transposed order), len, row = the
//          column; slot and pad_ mean nothing.  One lane group of k_attn_cols (fora_attn_bwd.h) per (column of this list,
//          head).  An empty column is in no list: its outputs are zeroed ahead of the kernels.
//   lng    the plan of PROPAGATE (fora_prop_plan.h) over the longer columns alone: their segments in chunks, and the records
//          of the combine.  A column of thousands of entries is many waves there, not one.
// The plan depends on col_ptr, the cap and the chunk size only, so it is made once per transposition and kept with it.
// Integer code, no HIP, no context -- fora_hip.hip owns buffers and launches, tests/attn_bwd_plan_check.cpp restates the split
// by brute force without a GPU.
#pragma once
#include "fora_attn_plan.h"

namespace fora {

struct AttnColPlan {
    std::vector<PropSeg> shrt;
    PropPlan lng;
    uint64_t columns = 0, max_col = 0;       // non-empty columns; the longest column
    uint64_t short_cols = 0, long_cols = 0;  // non-empty columns per path
};

// the segments of the columns longer than short_cap: what the chunk size of the long plan is resolved against
inline uint64_t attn_long_col_segs(const int64_t *col_ptr, int64_t n, uint32_t short_cap) {
    uint64_t s = 0;
    for (int64_t v = 0; v < n; v++) {
        const uint64_t len = (uint64_t)(col_ptr[v + 1] - col_ptr[v]);
        if (len > short_cap) s += (len + PROP_SEG - 1) / PROP_SEG;
    }
    return s;
}

// col_ptr: n + 1 ascending offsets from 0 (n below 2^31: a column is an int32 row of the plan); short_cap: attn_short_cap of
// the option; chunk_segs: segments per chunk of the long columns' product, at least 1
inline AttnColPlan attn_col_plan(const int64_t *col_ptr, int64_t n, uint32_t short_cap, uint64_t chunk_segs) {
    AttnColPlan p;
    if (n <= 0) return p;
    for (int64_t v = 0; v < n; v++) {
        const uint64_t len = (uint64_t)(col_ptr[v + 1] - col_ptr[v]);
        if (!len) continue;
        p.columns++;
        p.max_col = std::max(p.max_col, len);
        if (len <= short_cap) { p.shrt.push_back(PropSeg{col_ptr[v], (uint32_t)len, 0u, (int32_t)v, 0u}); p.short_cols++; }
        else p.long_cols++;
    }
    p.lng = prop_plan_if(col_ptr, (int)n, chunk_segs, [short_cap](int, uint64_t len) { return len > short_cap; });
    return p;
}

// how the lanes of k_attn_cols map to the w columns of a head's slice once the vector width V is chosen (attn_vec_width):
// prop_geom's lane groups -- G lanes (a power of two) hold a tile of G * V columns, a wave 64 / G units
inline PropGeom attn_cols_geom(uint32_t V, int w) {
    PropGeom g;
    g.V = V;
    const uint32_t lanes = ((uint32_t)w + V - 1) / V;
    g.G = 1;
    while (g.G < 64 && g.G < lanes) g.G *= 2;
    g.tiles = (lanes + g.G - 1) / g.G;
    g.segs_per_wave = 64 / g.G;
    return g;
}

} // namespace fora
