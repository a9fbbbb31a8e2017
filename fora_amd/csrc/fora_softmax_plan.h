// fora_softmax_plan.h -- the host side of ROW SOFTMAX (fora_hip_sparse_softmax, fora_hip_sparse_softmax_bwd; include/fora_hip.h):
// the segment list of fora_prop_plan.h split into the work lists of the two paths of fora_softmax.h.  A row of at most
// `softmax_short` entries (one segment) goes to the short list as it is; the segments of every longer row go to the long list,
// each told where its row's segments start in that list and how many they are, so that a wave finds the row's partial maxima
// and sums without a row table.  Integer code, no HIP, no context -- fora_hip.hip owns buffers and launches,
// tests/softmax_plan_check.cpp restates the split by brute force without a GPU.
#pragma once
#include "fora_prop_plan.h"

namespace fora {

constexpr uint32_t SMAX_SHORT_MAX = PROP_SEG; // the option "softmax_short" at most: a short row is one segment

inline uint32_t softmax_short_cap(int64_t option) { return (uint32_t)std::min<int64_t>(std::max<int64_t>(option, 0), SMAX_SHORT_MAX); }

// segs: the short list (n_short PropSeg as prop_plan made them; slot and pad_ mean nothing there), then the long list (n_long):
// slot = the place in the long list of the row's first segment, pad_ = the segments of the row.  Both keep row order.
struct SoftmaxLists { std::vector<PropSeg> segs; uint64_t n_short = 0, n_long = 0, short_rows = 0, long_rows = 0; };

// all: the segments of prop_plan(row_ptr, nq, ...), in row order; short_cap: softmax_short_cap of the option
inline SoftmaxLists softmax_lists(const std::vector<PropSeg> &all, const int64_t *row_ptr, uint32_t short_cap) {
    SoftmaxLists l;
    std::vector<PropSeg> lng;
    for (const PropSeg &s : all) {
        const uint64_t len = (uint64_t)(row_ptr[s.row + 1] - row_ptr[s.row]);
        if (len <= short_cap) { l.segs.push_back(s); l.short_rows++; continue; } // (<= PROP_SEG entries: the row's only segment)
        PropSeg t = s;
        const bool first = s.first == row_ptr[s.row];
        if (first) l.long_rows++;
        t.slot = first ? (uint32_t)lng.size() : lng.back().slot;
        t.pad_ = (uint32_t)((len + PROP_SEG - 1) / PROP_SEG);
        lng.push_back(t);
    }
    l.n_short = l.segs.size(); l.n_long = lng.size();
    l.segs.insert(l.segs.end(), lng.begin(), lng.end());
    return l;
}

} // namespace fora
