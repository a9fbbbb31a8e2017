// fora_propt_plan.h -- the host side of the transposition of PROPAGATE, TRANSPOSED (fora_hip_sparse_propagate_t; the contract is
// in include/fora_hip.h, the kernels in fora_propt.h): what the counts per node say about the work.  The counts become col_ptr
// by a prefix sum; every column's run of keys is then sorted on one of three tiers, chosen by the run's length and the option
// "propt_lds_cap".  Integer code, no HIP, no context -- fora_hip.hip owns buffers and launches, tests/propt_plan_check.cpp
// restates the split by brute force without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace fora {

constexpr uint32_t PROPT_SHORT = 64;     // keys of a run that one wave ranks with shuffles
constexpr uint32_t PROPT_LDS_MAX = 4096; // keys of a run that one workgroup sorts in LDS at most (32 KiB); the default of "propt_lds_cap"

// One column's run: keys [first, first + len) of the key buffer.
struct PropTRun { int64_t first; uint32_t len, pad_; };

// The three descriptor tables, one after the other in `runs` (so that one buffer holds them): short | lds | global.
struct PropTTiers {
    std::vector<PropTRun> runs;
    uint32_t n_short = 0, n_lds = 0, n_global = 0;
    uint32_t max_global = 0;            // the longest run of the global tier (0: none)
    uint64_t columns = 0, max_col = 0;  // columns with at least one entry; the longest column
};

// the option as a number of keys: below 0 counts as 0, above PROPT_LDS_MAX as that
inline uint32_t propt_lds_cap(int64_t option) { return (uint32_t)std::min<int64_t>(std::max<int64_t>(option, 0), PROPT_LDS_MAX); }

// the tier of a run of len keys: 0 none (nothing to sort), 1 short, 2 lds, 3 global.  A run longer than the cap goes to the
// global tier whatever its length: cap 0 sends every run of two keys or more there.
inline int propt_tier(uint64_t len, uint32_t cap) {
    if (len < 2) return 0;
    if (len > cap) return 3;
    return len <= PROPT_SHORT ? 1 : 2;
}

// counts per node -> col_ptr (n + 1 prefix sums); the total
inline uint64_t propt_scan(const uint32_t *cnt, int64_t n, int64_t *col_ptr) {
    int64_t at = 0;
    for (int64_t v = 0; v < n; v++) { col_ptr[v] = at; at += (int64_t)cnt[v]; }
    col_ptr[n] = at;
    return (uint64_t)at;
}

// at most this many runs need a descriptor: a run has two keys or more, and there are no more runs than nodes
inline uint64_t propt_max_runs(uint64_t n, uint64_t entries) { return std::min(n, entries / 2); }

inline PropTTiers propt_tiers(const int64_t *col_ptr, int64_t n, int64_t option) {
    PropTTiers t;
    const uint32_t cap = propt_lds_cap(option);
    for (int64_t v = 0; v < n; v++) {
        const uint64_t len = (uint64_t)(col_ptr[v + 1] - col_ptr[v]);
        t.columns += len != 0;
        t.max_col = std::max(t.max_col, len);
        switch (propt_tier(len, cap)) {
        case 1: t.n_short++; break;
        case 2: t.n_lds++; break;
        case 3: t.n_global++; t.max_global = std::max(t.max_global, (uint32_t)len); break;
        default: break;
        }
    }
    t.runs.resize((size_t)t.n_short + t.n_lds + t.n_global);
    size_t at[4] = {0, 0, t.n_short, (size_t)t.n_short + t.n_lds};
    for (int64_t v = 0; v < n; v++) {
        const uint64_t len = (uint64_t)(col_ptr[v + 1] - col_ptr[v]);
        const int tier = propt_tier(len, cap);
        if (tier) t.runs[at[tier]++] = PropTRun{col_ptr[v], (uint32_t)len, 0};
    }
    return t;
}

// ---- the sorting network of the lds and global tiers: a bitonic sort whose every compare-exchange puts the smaller key at
// the lower index, so that a run of any length sorts in place -- the positions from len up to the next power of two behave
// as keys above all others and never move, and an exchange whose upper index is one of them is skipped.  Stage k = 2, 4, ...
// (below 2 * len) starts with a flip (j == 0: index i of the lower half of a block of k against its mirror image in the
// upper half) and goes on with the strides j = k / 4, k / 8, ..., 1 (i against i + j).  Pair p of a step, p < P / 2 -- the one
// function the kernels and the CPU check both run (k and j are powers of two: shifts and masks, no divide):
#ifdef __HIPCC__
#define FORA_PROPT_HD __host__ __device__
#else
#define FORA_PROPT_HD
#endif
struct PropTPair { uint32_t lo, hi; };
FORA_PROPT_HD inline PropTPair propt_pair(uint32_t p, uint32_t k, uint32_t j) {
    if (!j) { const uint32_t b = p >> (__builtin_ctz(k) - 1), o = p & (k / 2 - 1u); return PropTPair{b * k + o, b * k + k - 1u - o}; }
    const int sh = __builtin_ctz(j);
    const uint32_t lo = ((p >> sh) << (sh + 1)) + (p & (j - 1u));
    return PropTPair{lo, lo + j};
}
// the power of two at or above len (len >= 1)
inline uint32_t propt_pow2(uint32_t len) { uint32_t P = 1; while (P < len) P *= 2; return P; }

} // namespace fora
