// fora_topk_plan.h -- the host side of the top-k sparse rows (the SPARSE RESULTS, TOP-K contract of include/fora_hip.h;
// DESIGN.md 5.14): what a row keeps, which tier selects it, how a batch's rows are cut into chunks of candidates, the
// clamping of the options "topk_lds_cap" and "topk_cand", and the sums of fora_topk_stats.  Integer code, no HIP, no
// context, no options struct -- fora_hip.hip owns buffers and launches, tests/topk_plan_check.cpp restates the plan by
// brute force without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace fora {

// ---- LDS tier: words of a row that one workgroup stages at most.  A workgroup may take all 160 KiB of a CU's LDS on
// gfx950; 18432 words are 144 KiB, which leaves 16 KiB for the kernel's own words (histogram, wave totals) and for the
// allocation granule.  The staged words are dynamic LDS sized by the longest staged row of the launch, so the occupancy
// follows the rows: a workgroup is 16 waves, two of them fill a CU's 32 wave slots, and they do so while the launch's
// longest staged row has at most 9216 words (72 KiB each); beyond that one workgroup of 16 waves runs per CU.
constexpr uint32_t TOPK_LDS_MAX = 18432;     // upper bound and default of "topk_lds_cap"
constexpr uint32_t TOPK_BLOCK = 1024;        // threads of a selection workgroup (k_topk_rows)

inline uint32_t topk_lds_cap(int64_t option) { return (uint32_t)std::min<int64_t>(std::max<int64_t>(option, 0), TOPK_LDS_MAX); }

// ---- what a row of `len` candidates keeps under k >= 1
inline bool topk_k_ok(int64_t k) { return k >= 1; }
inline uint64_t topk_held(uint64_t len, int64_t k) { return std::min<uint64_t>(len, (uint64_t)k); }

// ---- the tier of a row: it is copied (nothing to cut), selected in LDS, or selected from global memory
enum TopkTier : uint32_t { TOPK_COPY = 0, TOPK_LDS = 1, TOPK_GLOBAL = 2 };
inline TopkTier topk_tier(uint64_t len, int64_t k, uint32_t lds_cap /* clamped */) {
    if (len <= (uint64_t)k) return TOPK_COPY;
    return len <= lds_cap ? TOPK_LDS : TOPK_GLOBAL;
}

// ---- the candidate scratch: entries it holds.  option "topk_cand" > 0: that many; 0: what the free memory takes
// (free_entries); never more than the batch's candidates, never fewer than its longest row -- a row is never split.
inline uint64_t topk_cand_cap(int64_t option, uint64_t free_entries, uint64_t batch_total, uint64_t longest) {
    const uint64_t want = option > 0 ? (uint64_t)option : free_entries;
    return std::max<uint64_t>({longest, std::min(batch_total, want), 1});
}

// ---- a row of a chunk as the selection kernel reads it (uploaded as u64 words)
struct TopkRow {
    uint64_t cand;  // first candidate of the row in the scratch
    uint64_t out;   // first held entry of the row
    uint32_t len;   // candidates (the support; a row has fewer than 2^31)
    uint32_t keep;  // min(len, k)
};
static_assert(sizeof(TopkRow) == 24, "uploaded as three u64 words");

// ---- chunks of a batch: consecutive rows whose candidates fit the scratch together; the candidate bases restart at 0
// in every chunk.  A row longer than `cap` is a chunk of its own (the caller sizes the scratch by topk_cand_cap, so there
// is none).  Rows of len 0 ride with their neighbours.
struct TopkChunk {
    int r0 = 0, r1 = 0;      // rows [r0, r1) of the batch
    uint64_t entries = 0;    // candidates of the chunk
};
struct TopkBatchPlan {
    std::vector<TopkChunk> chunks;
    std::vector<uint64_t> cand; // per row of the batch: its candidate base inside its chunk
};
inline TopkBatchPlan topk_chunks(const uint32_t *len, int nb, uint64_t cap) {
    TopkBatchPlan p;
    p.cand.assign((size_t)std::max(nb, 0), 0);
    TopkChunk c;
    for (int i = 0; i < nb; i++) {
        if (i > c.r0 && c.entries + len[i] > cap) { c.r1 = i; p.chunks.push_back(c); c = TopkChunk{i, i, 0}; }
        p.cand[(size_t)i] = c.entries;
        c.entries += len[i];
    }
    if (nb > 0) { c.r1 = nb; p.chunks.push_back(c); }
    return p;
}

// ---- the first row of a chunk's k_sparse_write launch.  The kernel takes its row pointer for 16-byte aligned and picks
// its loads from (q * n) & 1, so a launch starts at an even row when n is odd; the row in front of an odd r0 rides along
// with a base at the scratch's end, where the kernel writes nothing.
inline int topk_launch_row(int r0, uint64_t n) { return (n & 1) ? (r0 & ~1) : r0; }

// ---- fora_topk_stats, summed over the live rows of a call
struct TopkSums {
    uint64_t support = 0, max_support = 0;
    int32_t cut_rows = 0, lds_rows = 0, global_rows = 0, chunks = 0;
    void add_row(uint64_t len, TopkTier t) {
        support += len; max_support = std::max(max_support, len);
        if (t != TOPK_COPY) cut_rows++;
        if (t == TOPK_LDS) lds_rows++;
        if (t == TOPK_GLOBAL) global_rows++;
    }
};

} // namespace fora
