// fora_sweep_plan.h -- the host side of SWEEP CUT (fora_hip_sweep_batch, fora_hip_seeds_sweep_batch; include/fora_hip.h):
// what a batch's support counts say about the work before its first launch -- every row's padded copy in the sort buffers
// and its profile in the held arrays (fora_rows.h), the tiles that one workgroup sorts in LDS, the rows of the global tier,
// and all of it as the words of one upload.  The records are the ones the kernels of fora_sweep.h read.  No HIP, no
// context, no options struct -- fora_hip.hip owns buffers and launches, tests/sweep_plan_check.cpp restates the plan by
// brute force without a GPU.
#pragma once
#include "fora_rows.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

namespace fora {

// Entries of a sort tile: key (8 bytes) + id (4 bytes) each, 48 KiB of LDS at 4096 -- under the 64 KiB a workgroup gets
// without asking, and three workgroups per CU inside its 160 KiB.
constexpr uint32_t SW_TILE_MAX = 4096;

struct SweepRowDesc { // a live row of the batch in progress
    int64_t tbase;    // first entry of its padded copy in the sort buffers
    int64_t hbase;    // first entry of its profile in the held arrays
    uint32_t len, P;  // support size; entries of the padded copy (a power of two >= len, 0 for an empty row)
    uint32_t L, pad_; // profile length, min(len, max_size)
};
struct SweepTile { int64_t base; uint32_t P, off; }; // tile of a row in the sort buffers: its first entry, the row's P, the tile's offset inside the row
struct SweepGRow { int64_t base; uint32_t P, pad_; }; // a row of the global tier
struct SweepRowOut { int64_t len, best; uint64_t cut, vol, den, edges; };

// the option sweep_lds_cap as entries of a sort tile: rounded down to a power of two, at most SW_TILE_MAX; 1: no LDS step at all
inline uint32_t sweep_tile(int64_t cap) {
    cap = std::min<int64_t>(cap, SW_TILE_MAX);
    uint32_t t = 1;
    while ((int64_t)t * 2 <= cap) t *= 2;
    return t;
}

// One upload: SweepRowDesc[nb] | tbase[nb] | SweepTile[tiles] | SweepGRow[grows], every record whole 64-bit words.  The view
// names the parts over a base pointer: Word = uint64_t to fill them on the host, const uint64_t to hand the parts of the
// uploaded copy to a kernel (a device pointer is only offset here, never read).
template <class Word> struct SweepDescView {
    template <class T> using As = typename std::conditional<std::is_const<Word>::value, const T, T>::type;
    Word *base; size_t nb, ntiles, ngrows;
    size_t words() const { return nb * (sizeof(SweepRowDesc) / 8 + 1) + ntiles * (sizeof(SweepTile) / 8) + ngrows * (sizeof(SweepGRow) / 8); }
    As<SweepRowDesc> *rows() const { return reinterpret_cast<As<SweepRowDesc> *>(base); }
    As<int64_t> *tbase() const { return reinterpret_cast<As<int64_t> *>(rows() + nb); }
    As<SweepTile> *tiles() const { return reinterpret_cast<As<SweepTile> *>(tbase() + nb); }
    As<SweepGRow> *grows() const { return reinterpret_cast<As<SweepGRow> *>(tiles() + ntiles); }
};
static_assert(sizeof(SweepRowDesc) % 8 == 0 && sizeof(SweepTile) % 8 == 0 && sizeof(SweepGRow) % 8 == 0, "records of whole words");

struct SweepBatchPlan {
    std::vector<SweepRowDesc> rd; // of the nb slots
    std::vector<int64_t> tbase;   // rd[i].tbase on its own: the `base` of k_sparse_write
    std::vector<SweepTile> tiles; // T >= 2: every row's padded copy in steps of T (a shorter row: one tile)
    std::vector<SweepGRow> grows; // the rows with P > T
    uint64_t tneed = 0;           // entries of the sort buffers
    uint32_t maxP = 0, maxL = 0;
    std::vector<uint64_t> pack;   // the upload
    template <class Word> SweepDescView<Word> view(Word *at) const { return SweepDescView<Word>{at, rd.size(), tiles.size(), grows.size()}; } // of a copy of the words at `at`
};

// The batch just closed: slot i has h_tot[i] entries over the threshold and is row at[i] of the caller (at null: row
// r0 + i); T: sweep_tile; max_size <= 0: profiles are not cut short.  Opens the batch in `lay` and places its rows there,
// in slot order.
inline SweepBatchPlan sweep_batch_plan(const uint32_t *h_tot, int nb, int64_t max_size, uint32_t T, RowLayout &lay, const int *at, int r0) {
    SweepBatchPlan p;
    p.rd.resize((size_t)nb);
    p.tbase.resize((size_t)nb);
    lay.begin_batch();
    for (int i = 0; i < nb; i++) {
        const uint32_t len = h_tot[i];
        uint32_t P = len ? 1 : 0;
        while (P < len) P *= 2; // (len <= n < 2^31)
        const uint32_t L = max_size > 0 ? (uint32_t)std::min<int64_t>(len, max_size) : len;
        p.rd[(size_t)i] = SweepRowDesc{(int64_t)p.tneed, lay.place(at ? at[i] : r0 + i, len, L), len, P, L, 0};
        p.tbase[(size_t)i] = (int64_t)p.tneed;
        if (P > T) p.grows.push_back(SweepGRow{(int64_t)p.tneed, P, 0});
        if (T >= 2) for (uint32_t off = 0; off < P; off += T) p.tiles.push_back(SweepTile{(int64_t)p.tneed + off, P, off});
        p.tneed += P;
        p.maxP = std::max(p.maxP, P); p.maxL = std::max(p.maxL, L);
    }
    p.pack.assign(p.view<uint64_t>(nullptr).words(), 0);
    const SweepDescView<uint64_t> v = p.view(p.pack.data());
    const auto put = [](void *to, const auto &from) { if (!from.empty()) memcpy(to, from.data(), from.size() * sizeof(from[0])); };
    put(v.rows(), p.rd);
    put(v.tbase(), p.tbase);
    put(v.tiles(), p.tiles);
    put(v.grows(), p.grows);
    return p;
}

} // namespace fora
