// fora_seeds_plan.h -- the host side of SEED SETS (fora_hip_query_seeds_batch and its sparse / sweep forms;
// include/fora_hip.h): what a call's set_ptr / seeds / weights say about the work before the first launch -- the checks of
// the sets, the weights at 2^-62, the slots of the seeds that run, the use list of every batch and the dangling seeds' terms
// as the words that are uploaded, the grid of k_seed_combine and the chunk of rows the sparse / sweep forms take at a time.
// Plain values in and out: no HIP, no context, no options struct -- fora_hip.hip owns buffers, uploads and launches,
// tests/seeds_plan_check.cpp restates the rules by brute force without a GPU.
#pragma once
#include "fora_consts.h"
#include "fora_rows.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <unordered_map>
#include <vector>

namespace fora {

// ---- set_ptr / ns / the seed count: the message to fail with, null when they are fine (ns == 0 is: nothing is read)
inline const char *seed_sets_error(const int64_t *set_ptr, const int32_t *seeds, int ns) {
    if (ns < 0) return "bad sets: negative count";
    if (ns == 0) return nullptr;
    if (!set_ptr || !seeds) return "bad sets: null set_ptr or seeds";
    if (set_ptr[0] != 0) return "set_ptr[0] must be 0";
    for (int g = 0; g < ns; g++)
        if (set_ptr[g + 1] <= set_ptr[g]) return set_ptr[g + 1] < set_ptr[g] ? "set_ptr decreases" : "empty seed set";
    if (set_ptr[ns] > 0x7FFFFFFF) return "more than 2^31 - 1 seeds in one call";
    return nullptr;
}

// ---- the weights at 2^-62, one word per listed seed.  weights null: seed j of a set of k gets floor(2^62 / k), the first
// 2^62 mod k seeds one unit more (the set sums to 2^62 exactly); given: S added left to right in doubles, then the floor of
// w / S * 2^62.  Returns the message to fail with (wfix is then unspecified), null when every set has its words.
inline const char *seed_weights(const int64_t *set_ptr, const double *weights, int ns, std::vector<uint64_t> &wfix) {
    wfix.assign((size_t)set_ptr[ns], 0);
    for (int g = 0; g < ns; g++) {
        const int64_t j0 = set_ptr[g], kg = set_ptr[g + 1] - j0;
        if (!weights) {
            const uint64_t base = FIX_ONE / (uint64_t)kg, rem = FIX_ONE % (uint64_t)kg;
            for (int64_t j = 0; j < kg; j++) wfix[(size_t)(j0 + j)] = base + ((uint64_t)j < rem ? 1 : 0);
            continue;
        }
        double S = 0;
        for (int64_t j = 0; j < kg; j++) {
            const double w = weights[j0 + j];
            if (!std::isfinite(w) || w < 0) return "seed weights must be finite and >= 0";
            S += w;
        }
        if (!(S > 0) || !std::isfinite(S)) return "the weights of a seed set must have a finite sum > 0";
        for (int64_t j = 0; j < kg; j++) wfix[(size_t)(j0 + j)] = (uint64_t)std::ldexp(weights[j0 + j] / S, 62);
    }
    return nullptr;
}

// ---- the slots: the seeds that run, in order of first appearance.  A dangling seed (an empty row of the graph's row_ptr)
// is its own whole answer and takes none: its term is w at the seed itself.  dedup: a live id runs once however often it is
// listed; without, every listed live seed has a slot of its own.
struct SeedUse { uint32_t set, slot; uint64_t w; }; // term of a set: the row of `slot` (of the call, then of its batch) times w / 2^62
struct SeedSlots {
    std::vector<int32_t> slot_src; // the seed of every slot
    std::vector<SeedUse> uses;     // the terms of the live seeds, by set
    std::vector<uint32_t> dang_set; std::vector<int32_t> dang_node; std::vector<uint64_t> dang_w; // the terms of the dangling ones, by set
    uint64_t distinct = 0;         // distinct ids listed, live or dangling
};
inline SeedSlots seed_slots(const int64_t *set_ptr, const int32_t *seeds, const uint64_t *wfix, int ns, const int64_t *row_ptr, bool dedup) {
    SeedSlots p;
    std::unordered_map<int32_t, uint32_t> slot_of; // seed id -> slot (with dedup; without: -> 0, the ids seen)
    for (int g = 0; g < ns; g++)
        for (int64_t j = set_ptr[g]; j < set_ptr[g + 1]; j++) {
            const int32_t s = seeds[j];
            const auto seen = slot_of.find(s);
            if (row_ptr[(size_t)s + 1] == row_ptr[(size_t)s]) {
                if (seen == slot_of.end()) slot_of.emplace(s, 0u);
                p.dang_set.push_back((uint32_t)g); p.dang_node.push_back(s); p.dang_w.push_back(wfix[(size_t)j]);
                continue;
            }
            uint32_t slot;
            if (dedup && seen != slot_of.end()) slot = seen->second;
            else {
                slot = (uint32_t)p.slot_src.size();
                p.slot_src.push_back(s);
                if (seen == slot_of.end()) slot_of.emplace(s, slot);
            }
            p.uses.push_back(SeedUse{(uint32_t)g, slot, wfix[(size_t)j]});
        }
    p.distinct = (uint64_t)slot_of.size();
    return p;
}

// ---- the two uploads, each a run of 64-bit words with 32-bit tables behind the 64-bit one.  A view names the tables over
// a base pointer: Word = uint64_t to fill the words on the host, const uint64_t to hand the tables of the uploaded copy to
// a kernel (a device pointer is only offset here, never read).
template <class Word> using HalfOf = typename std::conditional<std::is_const<Word>::value, const uint32_t, uint32_t>::type;

// The use list of one batch, sorted by set: use_w[U] (u64), then use_slot[U] | seg[T + 1] | set_id[T] (u32).  Set set_id[t]
// of the call has the uses [seg[t], seg[t + 1]) of the batch; T: the sets the batch touches.
template <class Word> struct SeedListView {
    Word *base; uint32_t U, T;
    static size_t words(uint32_t U, uint32_t T) { return (size_t)U + ((size_t)U + 2 * (size_t)T + 2) / 2; } // (U + 2 T + 1 u32, rounded up to whole words)
    Word *use_w() const { return base; }
    HalfOf<Word> *use_slot() const { return reinterpret_cast<HalfOf<Word> *>(base + U); }
    HalfOf<Word> *seg() const { return use_slot() + U; }
    HalfOf<Word> *set_id() const { return seg() + T + 1; }
};
// The dangling seeds' terms: w[nd] (u64), then set[nd] | node[nd] (32-bit)
template <class Word> struct SeedDanglingView {
    using Node = typename std::conditional<std::is_const<Word>::value, const int32_t, int32_t>::type;
    Word *base; size_t nd;
    static size_t words(size_t nd) { return 2 * nd; } // (2 nd halves are nd whole words)
    Word *w() const { return base; }
    HalfOf<Word> *set() const { return reinterpret_cast<HalfOf<Word> *>(base + nd); }
    Node *node() const { return reinterpret_cast<Node *>(set() + nd); }
};

// ---- the batches: slot s of the call runs in batch s / per as slot s % per.  Every batch gets its uses, in set order, as
// the words of its list.  nl: the slots of the call (every slot has a use, so no batch is empty)
struct SeedBatch {
    uint32_t U = 0, T = 0;
    std::vector<uint64_t> pack; // SeedListView::words(U, T)
    SeedListView<const uint64_t> list(const uint64_t *at) const { return SeedListView<const uint64_t>{at, U, T}; } // of a copy of the words at `at`
};
inline std::vector<SeedBatch> seed_batches(const std::vector<SeedUse> &uses, int nl, int per) {
    std::vector<SeedBatch> batches((size_t)((nl + per - 1) / per));
    std::vector<std::vector<SeedUse>> of(batches.size());
    for (const SeedUse &u : uses) of[u.slot / (uint32_t)per].push_back(SeedUse{u.set, u.slot % (uint32_t)per, u.w}); // (in set order)
    for (size_t bi = 0; bi < batches.size(); bi++) {
        const std::vector<SeedUse> &in = of[bi];
        SeedBatch &b = batches[bi];
        b.U = (uint32_t)in.size();
        for (uint32_t i = 0; i < b.U; i++) b.T += i == 0 || in[i].set != in[i - 1].set;
        b.pack.assign(SeedListView<uint64_t>::words(b.U, b.T), 0);
        const SeedListView<uint64_t> v{b.pack.data(), b.U, b.T};
        uint32_t t = 0;
        for (uint32_t i = 0; i < b.U; i++) {
            v.use_w()[i] = in[i].w;
            v.use_slot()[i] = in[i].slot;
            if (i == 0 || in[i].set != in[i - 1].set) { v.seg()[t] = i; v.set_id()[t++] = in[i].set; }
        }
        v.seg()[b.T] = b.U;
    }
    return batches;
}

inline std::vector<uint64_t> seed_dangling_pack(const SeedSlots &p) {
    const size_t nd = p.dang_set.size();
    std::vector<uint64_t> pack(SeedDanglingView<uint64_t>::words(nd), 0);
    const SeedDanglingView<uint64_t> v{pack.data(), nd};
    if (!nd) return pack;
    memcpy(v.w(), p.dang_w.data(), nd * 8);
    memcpy(v.set(), p.dang_set.data(), nd * 4);
    memcpy(v.node(), p.dang_node.data(), nd * 4);
    return pack;
}

// ---- the grid of k_seed_combine over a row of n ids: the compaction's (fora_rows.h) with SC_TILE and at least two tiles
inline CompactGeom seed_combine_geom(uint64_t n) { return compact_geom(n, SC_TILE, 2); }

// ---- rows of the finished block that the sparse / sweep forms compact (and sort) at a time: the option seeds_rows, at
// least 1, at most what a grid's y takes.  k_sparse_count / k_sparse_write choose between 16-byte and 8-byte loads from
// (q * n) & 1 and take their base for 16-byte aligned; a chunk starts at acc + r0 * n, an odd word when r0 * n is odd.  So
// with an odd n the count is rounded up to even: every chunk then starts at an even row.
inline int seeds_chunk(int64_t option, uint64_t n) {
    int64_t C = std::min<int64_t>(std::max<int64_t>(option, 1), 65534);
    if ((n & 1) && (C & 1)) C++;
    return (int)C;
}

} // namespace fora
