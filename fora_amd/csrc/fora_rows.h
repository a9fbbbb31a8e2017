// fora_rows.h -- the host side of "a result over rows, held on the device" (sparse rows, sweep profiles; DESIGN.md "Held
// rows"): rows in the caller's order, compacted batch by batch into arrays that grow as they fill.  No HIP, no context, no
// options struct -- fora_hip.hip owns buffers and launches, tests/rows_check.cpp restates the layout without a GPU.
#pragma once
#include "fora_consts.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace fora {

// ---- the `threshold` argument: valid up to 1 (a NaN is not), kept as a word at 2^-62, at least 1 -- zeros never pass
inline bool threshold_ok(double threshold) { return threshold <= 1.0; }
inline uint64_t threshold_word(double threshold) { return threshold > 0 ? std::max<uint64_t>(1, (uint64_t)std::ceil(std::ldexp(threshold, 62))) : 1; }

// ---- the compaction's grid over a slot of n ids: X workgroups of R ids each, R a multiple of the kernels' tile and at
// least min_tiles tiles; at most 1024 workgroups per slot (while n <= 1024 * 2^31: every n there is)
struct CompactGeom { uint32_t R = 0, X = 1; };
inline CompactGeom compact_geom(uint64_t n, uint32_t tile = SP_TILE, uint32_t min_tiles = 8) {
    const uint32_t R = (uint32_t)std::max<uint64_t>(min_tiles * (uint64_t)tile, ((n + 1023) / 1024 + tile - 1) / tile * tile);
    return CompactGeom{R, (uint32_t)((n + R - 1) / R)};
}

// ---- capacity to allocate when `need` entries no longer fit: rows_done of rows_all rows are placed, and what the rest
// will take is guessed from them (asked for again if the guess was short)
inline uint64_t grow_guess(uint64_t need, uint64_t rows_done, uint64_t rows_all) {
    const uint64_t guess = rows_done ? (uint64_t)((double)need / (double)rows_done * (double)rows_all * 1.125) + 1024 : need;
    return std::max<uint64_t>({need, guess, 1});
}

// ---- where every row of a call lies.  A batch's rows are placed when its counts are back: every row before them is
// known by then -- live rows of earlier batches, and one entry per row that no batch runs (a dangling source is its own
// whole answer).  Those entries are written last, from the list kept here.
struct RowLayout {
    std::vector<int64_t> row_ptr;  // nq + 1
    std::vector<int64_t> dang_at;  // entries of the dangling rows ...
    std::vector<int32_t> dang_src; // ... and their sources
    const int32_t *sources = nullptr; // of the nq rows; null: every row is placed, none is ever skipped
    int nq = 0, next_row = 0, batches = 0;
    uint64_t cur = 0;     // entries placed so far
    uint64_t written = 0; // how many of them, from the front, the device has been given to write: all that a grown array has to keep
    uint64_t max_row = 0, support = 0; // the longest support of a row; the supports summed

    void begin(const int32_t *sources_, int nq_) {
        *this = RowLayout{};
        sources = sources_; nq = nq_;
        row_ptr.assign((size_t)nq + 1, 0);
    }
    // rows up to (not including) row `upto` that no batch has placed yet: dangling sources, one entry each
    void skip_dangling(int upto) {
        for (; sources && next_row < upto; next_row++) {
            row_ptr[(size_t)next_row] = (int64_t)cur;
            dang_at.push_back((int64_t)cur);
            dang_src.push_back(sources[next_row]);
            cur += 1; support += 1;
            max_row = std::max<uint64_t>(max_row, 1);
        }
    }
    // a batch of live rows follows; the batches before it are on the device
    void begin_batch() { written = batches ? cur : 0; batches++; }
    // live row `row` of the caller (ascending from call to call): `len` entries pass the threshold, `held` of them are
    // kept (the sweep's max_size cuts a row short).  Returns its first entry.
    int64_t place(int row, uint64_t len, uint64_t held) {
        skip_dangling(row);
        const int64_t base = row_ptr[(size_t)row] = (int64_t)cur;
        cur += held; support += len;
        max_row = std::max(max_row, len);
        next_row = row + 1;
        return base;
    }
    // after the last batch: the trailing dangling rows, and the end of the last row
    void finish() {
        written = batches ? cur : 0;
        skip_dangling(nq);
        row_ptr[(size_t)nq] = (int64_t)cur;
    }
};

} // namespace fora
