// fora_attn_plan.h -- the host side of ATTENTION (fora_hip_sparse_attention; include/fora_hip.h): the caller's row_ptr split by
// the option "attn_short" into the work of the two paths of a call.
//   shrt   every row of at most `attn_short` entries, the empty ones included (whatever the option: an empty row is written
//          as +0.0 by the wave that finds it), as one PropSeg each -- first, len, row; slot and pad_ mean nothing.  One wave
//          of k_attn_short (fora_attn.h) per (row of this list, head).
//   lng    the plan of PROPAGATE (fora_prop_plan.h) over the longer rows alone: their segments in chunks of `prop_segs`, and
//          the row records of the combine.  The lists of SCORES and ROW SOFTMAX are made from these segments.
//   lrows  one PropSeg per longer row -- first, len, row -- for the kernel that rewrites the outputs of a NaN row.
// Integer code, no HIP, no context -- fora_hip.hip owns buffers and launches, tests/attn_plan_check.cpp restates the split by
// brute force without a GPU.
#pragma once
#include "fora_prop_plan.h"

namespace fora {

constexpr uint32_t ATTN_SHORT_MAX = PROP_SEG; // the option "attn_short" at most: a short row is one segment of every contract

inline uint32_t attn_short_cap(int64_t option) { return (uint32_t)std::min<int64_t>(std::max<int64_t>(option, 0), ATTN_SHORT_MAX); }

struct AttnPlan {
    std::vector<PropSeg> shrt, lrows;
    PropPlan lng;
    uint64_t entries = 0, segments = 0, max_row = 0; // of all rows, as PROPAGATE counts them
    uint64_t short_rows = 0, long_rows = 0;          // non-empty rows per path
};

// row_ptr has passed prop_row_ptr_ok; short_cap: attn_short_cap of the option; prop_segs: segments per chunk of the long
// rows' product, at least 1
inline AttnPlan attn_plan(const int64_t *row_ptr, int nq, uint32_t short_cap, uint64_t prop_segs) {
    AttnPlan p;
    if (nq <= 0) return p;
    p.entries = (uint64_t)row_ptr[nq];
    p.segments = prop_segments(row_ptr, nq);
    for (int i = 0; i < nq; i++) {
        const uint64_t len = (uint64_t)(row_ptr[i + 1] - row_ptr[i]);
        p.max_row = std::max(p.max_row, len);
        const PropSeg s{row_ptr[i], (uint32_t)std::min<uint64_t>(len, 0xFFFFFFFFull), 0u, i, 0u};
        if (len <= short_cap) { p.shrt.push_back(s); p.short_rows += len ? 1 : 0; }
        else { p.lrows.push_back(s); p.long_rows++; }
    }
    p.lng = prop_plan_if(row_ptr, nq, prop_segs, [short_cap](int, uint64_t len) { return len > short_cap; });
    return p;
}

// the widest of `widths` (descending, ending in 1) with which a lane may load adjacent columns of every head's slice of v:
// what prop_geom asks of base and pitch, and with more than one head of the slice width dv as well
inline uint32_t attn_vec_width(uint64_t v_addr, int64_t ldv, int dv, int heads, uint32_t elt_bytes, const uint32_t *widths, int nwidths) {
    const uint32_t V = prop_geom(v_addr, ldv, dv, elt_bytes, widths, nwidths).V;
    if (heads == 1 || dv % (int)V == 0) return V;
    for (int i = 0; i < nwidths; i++)
        if (widths[i] < V && dv % (int)widths[i] == 0) return prop_geom(v_addr, ldv, dv, elt_bytes, widths + i, nwidths - i).V;
    return 1;
}

} // namespace fora
