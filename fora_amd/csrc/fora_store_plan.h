// fora_store_plan.h -- the host side of the ROW STORE (fora_hip_store_put, _load, _take; include/fora_hip.h): what a row_ptr and
// a list of take indices have to satisfy, and the plan of a take.  A take copies rows of very different lengths (64 entries in a
// top-k store, thousands in a thresholded one), so the work is cut by OUTPUT entries, not by rows: span s is the output entries
// [s * span, (s + 1) * span), one workgroup's, and the plan tells it which taken rows meet it.
//   out_ptr  [nb + 1] the prefix sum of the taken rows' lengths: the row_ptr of the result
//   src      [nb]     where taken row i starts in the store
//   win      [spans + 1] win[s] = the taken row that holds output entry s * span (never an empty row); win[spans] = nb - 1.
// Output entry e of span s lies in the one row r of win[s] .. win[s + 1] with out_ptr[r] <= e < out_ptr[r + 1] -- the row that
// holds the span's last entry is not past the row that holds the next span's first -- and is entry src[r] + (e - out_ptr[r]) of
// the store.  Empty rows and rows that straddle spans are nothing special: an empty row is never the answer of that search.
// store_load checks its arrays over the same plan with the identity for the indices (rows == nullptr).
// Integer code, no HIP, no context -- fora_hip.hip owns buffers and launches, tests/store_plan_check.cpp restates the plan by
// brute force without a GPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace fora {

constexpr uint32_t STORE_SPAN_MIN = 64, STORE_SPAN_MAX = 1u << 16;
constexpr uint32_t STORE_SPAN_DEFAULT = 1024; // (the runs behind the choice)

// the option "take_span": a multiple of 64, at least 64
inline uint32_t store_span(int64_t option) {
    const int64_t v = std::min<int64_t>(std::max<int64_t>(option, STORE_SPAN_MIN), STORE_SPAN_MAX);
    return (uint32_t)(v / 64 * 64);
}

// a row_ptr of nrows rows: starts at 0 and never decreases (so no entry of it is negative)
inline bool store_row_ptr_ok(const int64_t *row_ptr, int64_t nrows) {
    if (!row_ptr || nrows < 0 || row_ptr[0] != 0) return false;
    for (int64_t i = 0; i < nrows; i++)
        if (row_ptr[i + 1] < row_ptr[i]) return false;
    return true;
}

// the place of the first take index outside [0, R); -1: every index names a row of the store
inline int64_t store_bad_index(const int64_t *rows, int64_t nb, int64_t R) {
    for (int64_t i = 0; i < nb; i++)
        if (rows[i] < 0 || rows[i] >= R) return i;
    return -1;
}

struct StorePlan {
    std::vector<int64_t> out_ptr, src; // nb + 1; nb
    std::vector<int64_t> win;          // spans + 1; empty without entries
    uint64_t entries = 0, max_row = 0, spans = 0;
    uint32_t span = 0;
    uint64_t max_win = 0;              // rows of the widest window, win[s] .. win[s + 1] inclusive
};

// store_ptr: the store's row_ptr (store_row_ptr_ok); rows: nb indices that passed store_bad_index, or nullptr for 0 .. nb - 1;
// span: store_span of the option
inline StorePlan store_take_plan(const int64_t *store_ptr, const int64_t *rows, int64_t nb, uint32_t span) {
    StorePlan p;
    p.span = span;
    p.out_ptr.assign((size_t)std::max<int64_t>(nb, 0) + 1, 0);
    p.src.assign((size_t)std::max<int64_t>(nb, 0), 0);
    for (int64_t i = 0; i < nb; i++) {
        const int64_t r = rows ? rows[i] : i;
        const uint64_t len = (uint64_t)(store_ptr[r + 1] - store_ptr[r]);
        p.src[(size_t)i] = store_ptr[r];
        p.out_ptr[(size_t)i + 1] = p.out_ptr[(size_t)i] + (int64_t)len;
        p.max_row = std::max(p.max_row, len);
    }
    p.entries = (uint64_t)p.out_ptr[(size_t)std::max<int64_t>(nb, 0)];
    if (!p.entries) return p;
    p.spans = (p.entries + span - 1) / span;
    p.win.assign((size_t)p.spans + 1, nb - 1);
    int64_t r = 0;
    for (uint64_t s = 0; s < p.spans; s++) { // (r only moves forward: O(nb + spans))
        const int64_t e = (int64_t)(s * span);
        while (p.out_ptr[(size_t)r + 1] <= e) r++;
        p.win[(size_t)s] = r;
    }
    for (uint64_t s = 0; s < p.spans; s++) p.max_win = std::max<uint64_t>(p.max_win, (uint64_t)(p.win[(size_t)s + 1] - p.win[(size_t)s]) + 1);
    return p;
}

// the search a lane makes: the row r of lo .. hi with ptr(r) <= e < ptr(r + 1), given that there is one (ptr(r): out_ptr[r],
// from the array or from a staged copy of the window).  constexpr: the kernels of fora_store.h call this very function.
template <typename Ptr>
constexpr int64_t store_find_row(Ptr ptr, int64_t lo, int64_t hi, int64_t e) {
    while (lo < hi) { // the smallest r with ptr[r + 1] > e
        const int64_t mid = lo + (hi - lo) / 2;
        if (ptr(mid + 1) > e) hi = mid; else lo = mid + 1;
    }
    return lo;
}

} // namespace fora
