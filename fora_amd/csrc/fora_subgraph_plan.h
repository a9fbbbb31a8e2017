// fora_subgraph_plan.h -- the host side of SUBGRAPH (fora_hip_sparse_subgraph, fora_hip_sparse_subgraph_fetch;
// include/fora_hip_ext.h): the arithmetic of the subgraph the graph induces on U, the columns of a compacted held result.
// The kept edges in row-major order are the SCANNED edges in order, filtered: the out-edges of U[0], U[1], .. concatenated,
// S of them, an edge kept exactly when its target is in U.  So the whole is one stream compaction over S:
//   rows     deg[j] = row_ptr[U[j] + 1] - row_ptr[U[j]]; scan_ptr = their exclusive sums in 64 bits, scan_ptr[nc] = S;
//            base[j] = row_ptr[U[j]] - scan_ptr[j], so that scanned edge p of row j is edge base[j] + p of the graph
//   count    span s is the scanned edges [s * span, (s + 1) * span) below S (the option "sub_span"); its rows are
//            sub_find_row(first edge) .. sub_find_row(last edge); cnt[s] = its edges whose target's bit is set in the bitmap
//   scan     off[s] = cnt[0] + .. + cnt[s - 1] in 64 bits; their sum is the edges of the subgraph
//   write    the k-th kept edge of span s goes to place off[s] + k: sub_col = cols_rank of the target, sub_eid = its place in
//            the graph's col; sub_ptr[j] = off[s] + the kept edges of the span in front of scan_ptr[j] for every row j of
//            sub_rows_from(span's first edge) .. sub_rows_from(the next span's) -- rows without edges share their start with
//            their successor and are all in that range; the last span takes the rows at S and sub_ptr[nc] on top
// Integer code, no HIP, no context -- fora_hip.hip owns buffers and launches, the kernels of fora_subgraph.h call sub_find_row
// and sub_rows_from themselves, tests/subgraph_plan_check.cpp restates the four steps through these functions and holds them
// to brute force without a GPU.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "fora_cols_plan.h"  // the bitmap of U and cols_rank
#include "fora_store_plan.h" // store_find_row

namespace fora {

// the LDS of a workgroup of the write pass holds span + 1 prefix sums of 4 bytes: 1 KiB at the minimum, 32 KiB at the maximum
constexpr uint32_t SUB_SPAN_MIN = 256, SUB_SPAN_MAX = 8192;
constexpr uint32_t SUB_SPAN_DEFAULT = 2048; // PROVISIONAL and unmeasured: chosen before any run (DESIGN.md 5.23 says what is to replace it)

// the option "sub_span": a power of two from 256 to 8192 scanned edges; other values are clamped and rounded down to one
inline uint32_t sub_span(int64_t option) {
    const uint32_t v = (uint32_t)std::min<int64_t>(std::max<int64_t>(option, SUB_SPAN_MIN), SUB_SPAN_MAX);
    uint32_t p = SUB_SPAN_MIN;
    while (p * 2 <= v) p *= 2;
    return p;
}

// spans of `span` scanned edges over S of them: the counts the scan adds up
constexpr uint64_t sub_spans(uint64_t S, uint32_t span) { return (S + span - 1) / span; }

// the row r of lo .. hi with ptr(r) <= p < ptr(r + 1), given that there is one (ptr(r): scan_ptr[r]); rows without edges are
// stepped over.  The search of the row store's take, and constexpr like it: the kernels of fora_subgraph.h call this function.
template <typename Ptr>
constexpr int64_t sub_find_row(Ptr ptr, int64_t lo, int64_t hi, int64_t p) { return store_find_row(ptr, lo, hi, p); }

// the smallest j of 0 .. nc with ptr(j) >= x, for 0 <= x <= S = ptr(nc) and S > 0: the first row whose scanned edges start
// at x or behind it (nc: none does).  Rows j of [sub_rows_from(a), sub_rows_from(b)) are those with a <= ptr(j) < b.
template <typename Ptr>
constexpr int64_t sub_rows_from(Ptr ptr, int64_t nc, int64_t x) { return x ? sub_find_row(ptr, 0, nc - 1, x - 1) + 1 : 0; }

// is node t in U?  (t < 64 * the bitmap's words)
constexpr bool sub_member(uint64_t word, uint32_t t) { return (word >> (t & 63)) & 1; }

} // namespace fora
