// fora_flush_plan.h -- the arithmetic of the line-aligned flush of a wave's result stage (stage_flush<.., ONE = true, G>,
// fora_kernels.h; k_walk_dg).  A flush has counted the stage's results per bin and ranked every result inside its bin.  With
// G > 0 (results of 8 bytes per aligned line: 8 = 64 bytes, 16 = 128) it then sends, per bin, only what ends on a line
// boundary of the workgroup's sub-bucket and keeps the rest -- at most G - 1 results a bin -- in the stage:
//   head   what brings the sub-bucket's fill back to a multiple of G (0 once it is one)
//   send   s = c < head ? 0 : head + (c - head) / G * G of the bin's c results; c - s stay
//   full   the kept results of all bins together would exceed the cap: this flush sends every result, unaligned; the next
//          one re-aligns through head.  So does the kernel's closing flush.
//   slots  the stage is rebuilt from registers: the kept results, by bin, in slots 0 .. kept - 1, the sent ones, by bin,
//          behind them -- consecutive lanes then store to consecutive bucket slots, and the kept ones are where the next
//          results are appended.  One 32-bit word per bin carries what an entry needs to find its slot (FlushBin).
// The fill is read before the returning add that reserves s: once every sub-bucket stands on a multiple of G all adds are
// multiples of G, so the read cannot be stale in a way that matters; before that (fills left by the indexed walks, a full
// flush) a stale read costs one unaligned run and no result -- a run goes where the add's return value says.
// Integer code, no HIP, no context: stage_flush calls these very functions, tests/flush_plan_check.cpp drives them over
// many flushes without a GPU.
#pragma once
#include <stdint.h>

namespace fora {

constexpr uint32_t FLUSH_SLOT_BITS = 9;                 // a stage holds at most 511 results
constexpr uint32_t FLUSH_SLOT_MASK = (1u << FLUSH_SLOT_BITS) - 1;
constexpr uint32_t FLUSH_LINE_MAX = 16;                  // results of the longest line an arm aligns to (128 bytes): plan_workspace rounds a sub-bucket's capacity to it
constexpr uint32_t FLUSH_ROOM = 64;                     // the emit path appends up to a wave's 64 results before it flushes

// results that bring a sub-bucket standing at `fill` to the next multiple of G
constexpr uint32_t flush_head(uint32_t fill, uint32_t G) { return (G - fill % G) % G; }

// results of a bin's c that an aligned flush sends to a sub-bucket standing at `fill`
constexpr uint32_t flush_send(uint32_t c, uint32_t fill, uint32_t G) {
    const uint32_t head = flush_head(fill, G);
    return c < head ? 0u : head + (c - head) / G * G;
}

// the cap on the results a flush keeps: the option "walk_flush_keep" (0: half the stage), never more than leaves the emit
// path its room
constexpr uint32_t flush_keep_cap(uint32_t stage, uint32_t option) {
    const uint32_t k = option ? option : stage / 2;
    return k < stage - FLUSH_ROOM ? k : stage - FLUSH_ROOM;
}

// progress rule: keeping `kept` results would leave too few free slots -- send everything
constexpr bool flush_full(uint32_t kept, uint32_t cap) { return kept > cap; }

// a bin's word: results sent | first slot of its kept results | first slot of its sent ones less the number kept in all
struct FlushBin {
    uint32_t w;
    static constexpr FlushBin make(uint32_t sent, uint32_t kept_before, uint32_t sent_before) {
        return FlushBin{sent | (kept_before << FLUSH_SLOT_BITS) | (sent_before << (2 * FLUSH_SLOT_BITS))};
    }
    constexpr uint32_t sent() const { return w & FLUSH_SLOT_MASK; }
    constexpr uint32_t kept_before() const { return (w >> FLUSH_SLOT_BITS) & FLUSH_SLOT_MASK; }
    constexpr uint32_t sent_before() const { return w >> (2 * FLUSH_SLOT_BITS); }
    // leaves with this flush: the bin's first sent() results by rank
    constexpr bool sends(uint32_t rank) const { return rank < sent(); }
    // new stage slot of the bin's result of that rank; kept: the results all bins keep together
    constexpr uint32_t slot(uint32_t rank, uint32_t kept) const {
        return sends(rank) ? kept + sent_before() + rank : kept_before() + (rank - sent());
    }
};

} // namespace fora
