// fora_subgraph_prop_plan.h -- the host side of SUBGRAPH PRODUCTS (fora_hip_subgraph_propagate, fora_hip_subgraph_propagate_t,
// fora_hip_subgraph_transpose_fetch; include/fora_hip_gnn.h): what the held subgraph's offsets say about the work of a product.
//   the option   "sub_short" as a number of entries, 0 .. 256 (sub_short_cap)
//   the split    an output row (a row of sub_ptr forward, a column of in_ptr transposed) of at most that many entries, the empty
//                ones included whatever the option, is summed and written by k_sub_agg in one pass -- one segment of the
//                contract, so its sum from +0.0 in entry order is the contract's; a longer one goes through the plan of
//                PROPAGATE (fora_prop_plan.h) made for the longer ones alone, whose records name the rows they write
//   the transposition, restated on the host: column v lists the edges whose target is v by ascending place in sub_col -- a
//                stable counting sort of the places by target; the device builds the same arrays with integer atomics and a
//                sort of (row << 32 | place in the row) keys, which ascend exactly as the places do
// Integer code, no HIP, no context -- fora_hip.hip owns buffers and launches, tests/subgraph_prop_plan_check.cpp holds these
// functions to brute force without a GPU.
#pragma once
#include "fora_prop_plan.h"

namespace fora {

constexpr uint32_t SUB_SHORT_MAX = PROP_SEG; // the option "sub_short" at most: a short row is one segment of the contract
constexpr uint32_t SUB_SHORT_DEFAULT = SUB_SHORT_MAX;

inline uint32_t sub_short_cap(int64_t option) { return (uint32_t)std::min<int64_t>(std::max<int64_t>(option, 0), SUB_SHORT_MAX); }

// which path owns an output row of len entries: true k_sub_agg, false the long path
constexpr bool sub_row_short(uint64_t len, uint32_t cap) { return len <= cap; }

struct SubSplit { uint64_t short_rows = 0, long_rows = 0, long_segs = 0, max_row = 0; }; // (short_rows: the empty ones included)
inline SubSplit sub_split(const int64_t *ptr, int rows, uint32_t cap) {
    SubSplit s;
    for (int i = 0; i < rows; i++) {
        const uint64_t len = (uint64_t)(ptr[i + 1] - ptr[i]);
        s.max_row = std::max(s.max_row, len);
        if (sub_row_short(len, cap)) s.short_rows++;
        else { s.long_rows++; s.long_segs += (len + PROP_SEG - 1) / PROP_SEG; }
    }
    return s;
}

// the plan of the long path: PROPAGATE's over the rows k_sub_agg leaves out, in chunks of prop_segs segments (at least 1)
inline PropPlan sub_long_plan(const int64_t *ptr, int rows, uint32_t cap, uint64_t prop_segs) {
    return prop_plan_if(ptr, rows, prop_segs, [cap](int, uint64_t len) { return !sub_row_short(len, cap); });
}

// the transposition of a CSR of `rows` rows and as many columns: in_ptr [rows + 1], in_row and in_pos [edges]; false when a
// column index lies outside [0, rows)
inline bool sub_transpose_host(const int64_t *ptr, const int32_t *col, int rows, std::vector<int64_t> &in_ptr, std::vector<int32_t> &in_row,
                               std::vector<int64_t> &in_pos) {
    const int64_t edges = rows > 0 ? ptr[rows] : 0;
    in_ptr.assign((size_t)std::max(rows, 0) + 1, 0);
    in_row.assign((size_t)edges, 0);
    in_pos.assign((size_t)edges, 0);
    for (int64_t e = 0; e < edges; e++) {
        if (col[e] < 0 || col[e] >= rows) return false;
        in_ptr[(size_t)col[e] + 1]++;
    }
    for (int v = 0; v < rows; v++) in_ptr[(size_t)v + 1] += in_ptr[(size_t)v];
    std::vector<int64_t> next(in_ptr.begin(), in_ptr.end() - 1);
    for (int i = 0; i < rows; i++)
        for (int64_t e = ptr[i]; e < ptr[i + 1]; e++) {
            const int64_t p = next[(size_t)col[e]]++;
            in_row[(size_t)p] = i;
            in_pos[(size_t)p] = e;
        }
    return true;
}

// the key the device sorts a column's run by: (row << 32) | place inside the row.  Rows are contiguous in sub_col, so keys
// ascend exactly as places do -- two entries of one row with one target (a multi-edge) differ in their low word
constexpr uint64_t sub_key(uint32_t row, uint64_t place_in_row) { return ((uint64_t)row << 32) | place_in_row; }

} // namespace fora
