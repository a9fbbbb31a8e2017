// fora_store.h -- the kernels of the ROW STORE (fora_hip_store_take, fora_hip_store_load; the contract is in include/fora_hip.h).
//   k_store_take   a load-balanced segmented copy: rows of the store, in the caller's order, become the held sparse result.
//   k_store_check  the validation of store_load: every id in [0, n), ids strictly ascending inside a row; the smallest bad
//                  entry comes back through an integer atomic minimum.
// Both run over the span plan of fora_store_plan.h: a workgroup owns `span` consecutive OUTPUT entries, whatever rows they
// belong to -- a row of 64 entries and one of 17 000 cost what their entries cost, and neither one wave nor one workgroup per
// row would be right for both.  The rows that meet a span are its window win[s] .. win[s + 1]; the workgroup stages the
// window's slice of out_ptr (and of src) in LDS when it has at most STORE_WIN_LDS rows, and every lane finds its entry's row
// there by bisection (store_find_row, the host plan's own function).  A wider window -- a span met by hundreds of empty rows --
// is searched in global memory instead; same result.  Consecutive lanes write consecutive entries and, inside a row, read
// consecutive entries, so a wave's 64 ids are one 256-byte piece and its 64 words one 512-byte piece wherever a row does not
// end; a row's first id is only 4-byte aligned, which is why no lane reads more than its own entry.
// No scratch, nothing spilled: a lane holds STORE_ILP entries' addresses and values at a time.
#pragma once
#include "fora_kernels.h" // BLOCK
#include "fora_store_plan.h"

namespace fora {

constexpr uint32_t STORE_WIN_LDS = 512; // rows of a window staged in LDS at most: (2 * 512 + 1) * 8 bytes
constexpr int STORE_ILP = 4;            // entries a lane has in flight

struct StoreWin { int64_t lo, hi; bool staged; };

// the window of span s; staged: s_ptr[i] = out_ptr[lo + i] for i = 0 .. rows, and (src given) s_src[i] = src[lo + i] for i < rows.
// Every thread of the workgroup calls it; the barrier is inside.
__device__ __forceinline__ StoreWin store_stage(const int64_t *__restrict__ out_ptr, const int64_t *__restrict__ src, const int64_t *__restrict__ win, uint64_t s,
                                                int64_t *s_ptr, int64_t *s_src) {
    StoreWin w;
    w.lo = win[s]; w.hi = win[s + 1];
    const uint64_t rows = (uint64_t)(w.hi - w.lo) + 1;
    w.staged = rows <= STORE_WIN_LDS;
    __syncthreads(); // (the span before this one has been read)
    if (w.staged) {
        for (uint32_t i = threadIdx.x; i <= rows; i += BLOCK) {
            s_ptr[i] = out_ptr[w.lo + i];
            if (src && i < rows) s_src[i] = src[w.lo + i];
        }
        __syncthreads();
    }
    return w;
}
// the row of output entry e inside the window, and where the row starts in the output
__device__ __forceinline__ int64_t store_row_of(const StoreWin &w, const int64_t *__restrict__ out_ptr, const int64_t *s_ptr, int64_t e, int64_t &row_first) {
    int64_t r;
    if (w.staged) {
        r = store_find_row([&](int64_t i) { return s_ptr[i - w.lo]; }, w.lo, w.hi, e);
        row_first = s_ptr[r - w.lo];
    } else {
        r = store_find_row([&](int64_t i) { return out_ptr[i]; }, w.lo, w.hi, e);
        row_first = out_ptr[r];
    }
    return r;
}

// out_ids / out_fix [entries] (of room out_cap) = the taken rows one after the other; ids / fix: the store (store_entries of them)
__global__ __launch_bounds__(BLOCK) void k_store_take(const int64_t *__restrict__ out_ptr, const int64_t *__restrict__ src, const int64_t *__restrict__ win,
                                                      uint64_t spans, uint64_t entries, uint32_t span, const int32_t *__restrict__ ids, const uint64_t *__restrict__ fix,
                                                      uint64_t store_entries, int32_t *__restrict__ out_ids, uint64_t *__restrict__ out_fix, uint64_t out_cap) {
    __shared__ int64_t s_ptr[STORE_WIN_LDS + 1];
    __shared__ int64_t s_src[STORE_WIN_LDS];
    const uint64_t lim = entries < out_cap ? entries : out_cap;
    for (uint64_t s = blockIdx.x; s < spans; s += gridDim.x) {
        const StoreWin w = store_stage(out_ptr, src, win, s, s_ptr, s_src);
        const uint64_t e0 = s * span, e1 = e0 + span < lim ? e0 + span : lim;
        for (uint64_t eb = e0 + threadIdx.x; eb < e1; eb += (uint64_t)BLOCK * STORE_ILP) {
            uint64_t from[STORE_ILP];
            int32_t id[STORE_ILP];
            uint64_t wd[STORE_ILP];
#pragma unroll
            for (int j = 0; j < STORE_ILP; j++) {
                const uint64_t e = eb + (uint64_t)j * BLOCK;
                from[j] = ~0ull;
                if (e < e1) {
                    int64_t first;
                    const int64_t r = store_row_of(w, out_ptr, s_ptr, (int64_t)e, first);
                    from[j] = (uint64_t)((w.staged ? s_src[r - w.lo] : src[r]) + ((int64_t)e - first));
                }
            }
#pragma unroll
            for (int j = 0; j < STORE_ILP; j++)
                if (from[j] < store_entries) { id[j] = ids[from[j]]; wd[j] = fix[from[j]]; }
#pragma unroll
            for (int j = 0; j < STORE_ILP; j++)
                if (from[j] < store_entries) { const uint64_t e = eb + (uint64_t)j * BLOCK; out_ids[e] = id[j]; out_fix[e] = wd[j]; }
        }
    }
}

// row_ptr / win: the identity plan over the arrays under test (src == row_ptr); *bad = min(*bad, e) for every entry e whose id
// is outside [0, n) or not above the id before it in the same row.  *bad starts at ~0.
__global__ __launch_bounds__(BLOCK) void k_store_check(const int64_t *__restrict__ row_ptr, const int64_t *__restrict__ win, uint64_t spans, uint64_t entries, uint32_t span,
                                                       const int32_t *__restrict__ ids, uint32_t n, unsigned long long *bad) {
    __shared__ int64_t s_ptr[STORE_WIN_LDS + 1];
    for (uint64_t s = blockIdx.x; s < spans; s += gridDim.x) {
        const StoreWin w = store_stage(row_ptr, nullptr, win, s, s_ptr, nullptr);
        const uint64_t e0 = s * span, e1 = e0 + span < entries ? e0 + span : entries;
        for (uint64_t e = e0 + threadIdx.x; e < e1; e += BLOCK) {
            int64_t first;
            (void)store_row_of(w, row_ptr, s_ptr, (int64_t)e, first);
            const int32_t id = ids[e];
            const bool ok = (uint32_t)id < n && ((int64_t)e == first || ids[e - 1] < id);
            if (!ok) atomicMin(bad, (unsigned long long)e);
        }
    }
}

} // namespace fora
