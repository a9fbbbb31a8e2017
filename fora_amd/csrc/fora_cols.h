// fora_cols.h -- the kernels of COLUMNS (fora_hip_sparse_compact; the contract is in include/fora_hip.h, the arithmetic in
// fora_cols_plan.h): the held ids re-expressed as ranks in U, the ascending set of the distinct ids among them.
//   k_cols_mark     one lane per held entry sets its id's bit in a bitmap over the n nodes (zeroed in front of it)
//   k_cols_totals   a workgroup counts the set bits of `block` consecutive words: one total per block
//   k_cols_scan     ONE workgroup scans the totals exclusively, BLOCK at a time, and writes nc = |U|
//   k_cols_list     a workgroup counts its block again, scans the counts (wave prefix sums, LDS across the waves), writes the
//                   rank of every word's first set bit and the ids of the set bits, ascending, to cols
//   k_cols_relabel  one lane per held entry: its id becomes cols_rank(wrank[word], word, bit)
// Integers only, flat over the entries: no row structure is needed.  The scan is three launches on purpose: no workgroup ever
// waits for another one -- no look-back chain, no flags, no spinning.  Every kernel strides over its work, so the grid is a
// matter of speed only; every store is inside the bounds its caller passes (an id outside [0, n) is skipped, a rank outside
// the room of cols is not written).  OR is idempotent and order-free: the bitmap does not depend on the order of arrival.
// No scratch, nothing spilled.
#pragma once
#include "fora_kernels.h" // BLOCK, block_excl_scan
#include "fora_cols_plan.h"

namespace fora {

// PPR rows share their hubs: most ids of a batch are marked already when a lane meets them, so the lane reads the word first
// and issues the atomic only when its bit is still clear (a stale read costs one atomic more, never a wrong bit).
__global__ __launch_bounds__(BLOCK) void k_cols_mark(const int32_t *__restrict__ ids, uint64_t entries, uint32_t n, unsigned long long *bitmap) {
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < entries; e += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t id = (uint32_t)ids[e];
        if (id >= n) continue;
        const uint64_t w = cols_word_of(id), m = cols_mask_of(id);
        if (!(bitmap[w] & m)) atomicOr(&bitmap[w], (unsigned long long)m);
    }
}

// total[b] = the set bits of words [b * block, (b + 1) * block) below `words`
__global__ __launch_bounds__(BLOCK) void k_cols_totals(const unsigned long long *__restrict__ bitmap, uint64_t words, uint32_t block, uint64_t blocks, uint32_t *__restrict__ total) {
    __shared__ uint32_t s_w[BLOCK / 64];
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint64_t w0 = b * block;
        uint32_t cnt = 0;
        for (uint32_t i = threadIdx.x; i < block; i += BLOCK)
            if (w0 + i < words) cnt += cols_popcount(bitmap[w0 + i]);
        uint32_t tot;
        (void)block_excl_scan(cnt, s_w, tot);
        if (threadIdx.x == 0) total[b] = tot;
    }
}

// off[b] = total[0] + .. + total[b - 1]; *nc = the sum of all.  One workgroup: launched with a grid of one.
__global__ __launch_bounds__(BLOCK) void k_cols_scan(const uint32_t *__restrict__ total, uint64_t blocks, uint32_t *__restrict__ off, unsigned long long *nc) {
    __shared__ uint32_t s_w[BLOCK / 64];
    if (blockIdx.x) return;
    uint32_t carry = 0;
    for (uint64_t b0 = 0; b0 < blocks; b0 += BLOCK) { // (more totals than threads: the loop)
        const uint64_t b = b0 + threadIdx.x;
        const uint32_t t = b < blocks ? total[b] : 0;
        uint32_t tot;
        const uint32_t x = block_excl_scan(t, s_w, tot);
        if (b < blocks) off[b] = carry + x;
        carry += tot;
    }
    if (threadIdx.x == 0) *nc = carry;
}

// wrank[w] = the rank of word w's first set bit; cols[wrank[w] ..] = the ids of its set bits, ascending (room: cap entries)
__global__ __launch_bounds__(BLOCK) void k_cols_list(const unsigned long long *__restrict__ bitmap, uint64_t words, uint32_t block, uint64_t blocks,
                                                     const uint32_t *__restrict__ off, uint32_t *__restrict__ wrank, int32_t *__restrict__ cols, uint64_t cap) {
    __shared__ uint32_t s_w[BLOCK / 64];
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint64_t w0 = b * block;
        uint32_t carry = off[b];
        for (uint32_t i0 = 0; i0 < block; i0 += BLOCK) { // (uniform bounds: every thread meets the scan's barriers)
            const uint64_t w = w0 + i0 + threadIdx.x;
            const bool mine = i0 + threadIdx.x < block && w < words;
            uint64_t word = mine ? bitmap[w] : 0;
            uint32_t tot;
            uint32_t r = carry + block_excl_scan(cols_popcount(word), s_w, tot);
            carry += tot;
            if (!mine) continue;
            wrank[w] = r;
            for (; word; word &= word - 1, r++)
                if (r < cap) cols[r] = (int32_t)(w * 64 + (uint64_t)(__ffsll((long long)word) - 1));
        }
    }
}

// ids[e] = the rank of ids[e] in U
__global__ __launch_bounds__(BLOCK) void k_cols_relabel(int32_t *__restrict__ ids, uint64_t entries, uint32_t n, const unsigned long long *__restrict__ bitmap,
                                                        const uint32_t *__restrict__ wrank) {
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < entries; e += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t id = (uint32_t)ids[e];
        if (id >= n) continue;
        const uint64_t w = cols_word_of(id);
        ids[e] = (int32_t)cols_rank(wrank[w], bitmap[w], id & 63);
    }
}

} // namespace fora
