// fora_cols_plan.h -- the host side of COLUMNS (fora_hip_sparse_compact, fora_hip_sparse_cols_fetch; include/fora_hip.h): the
// arithmetic of re-expressing the held sparse result over its own columns.  U, the ascending set of the distinct ids among the
// held entries, is found through a bitmap over the n nodes, 64 to a word:
//   mark     bit (id & 63) of word (id >> 6) is set for every held id
//   totals   block b of `block` consecutive words (the option "cols_block") holds total[b] set bits
//   scan     off[b] = total[0] + .. + total[b - 1]; their sum is nc = |U|
//   list     wrank[w] = off[w / block] + the set bits of the block's words in front of w: the rank of word w's first set bit;
//            the ids of the set bits, w * 64 + bit, go to cols[wrank[w] ..] in ascending order
//   relabel  id' = cols_rank(wrank[id >> 6], word, id & 63): the rank of id in U
// The relabelling is monotone, so ids that ascend strictly inside a row still do.
// Integer code, no HIP, no context -- fora_hip.hip owns buffers and launches, the kernels of fora_cols.h call cols_rank itself,
// tests/cols_plan_check.cpp restates the five steps through these functions and holds them to brute force without a GPU.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace fora {

constexpr uint32_t COLS_BLOCK_MIN = 1, COLS_BLOCK_MAX = 4096;
constexpr uint32_t COLS_BLOCK_DEFAULT = 256;  // (the runs behind the choice)

// words of the bitmap over n nodes
constexpr uint64_t cols_words(uint64_t n) { return (n + 63) / 64; }

// the option "cols_block": a power of two from 1 to 4096 words; other values are clamped and rounded down to one
inline uint32_t cols_block(int64_t option) {
    const uint32_t v = (uint32_t)std::min<int64_t>(std::max<int64_t>(option, COLS_BLOCK_MIN), COLS_BLOCK_MAX);
    uint32_t p = 1;
    while (p * 2 <= v) p *= 2;
    return p;
}

// blocks of `block` words over `words` words: the totals the scan adds up
constexpr uint64_t cols_blocks(uint64_t words, uint32_t block) { return (words + block - 1) / block; }

// where id lives in the bitmap
constexpr uint64_t cols_word_of(uint32_t id) { return id >> 6; }
constexpr uint64_t cols_mask_of(uint32_t id) { return 1ull << (id & 63); }

// set bits of a word
constexpr uint32_t cols_popcount(uint64_t word) { return (uint32_t)__builtin_popcountll(word); }

// the rank in U of the id at bit `bit` of a word whose first set bit has rank wrank: the set bits below it counted on top.
// constexpr: k_cols_relabel (fora_cols.h) calls this very function.
constexpr uint32_t cols_rank(uint32_t wrank, uint64_t word, uint32_t bit) { return wrank + cols_popcount(word & ((1ull << bit) - 1)); }

} // namespace fora
