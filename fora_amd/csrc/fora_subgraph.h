// fora_subgraph.h -- the kernels of SUBGRAPH (fora_hip_sparse_subgraph; the contract is in include/fora_hip_ext.h, the arithmetic
// in fora_subgraph_plan.h): the CSR of the subgraph the graph induces on U, the columns of a compacted held result, as one
// stream compaction over the S scanned edges -- the out-edges of U[0], U[1], .. concatenated.
//   k_sub_row_totals  a workgroup adds up the out-degrees of BLOCK consecutive rows of U: one total per block
//   k_sub_scan        ONE workgroup scans totals (of rows, of spans) exclusively in 64 bits, BLOCK at a time, and writes their sum
//   k_sub_row_list    a workgroup takes its degrees again, scans them, writes scan_ptr and base (and scan_ptr[nc] = S)
//   k_sub_count       a workgroup takes one span of scanned edges: each lane finds its edge's row in the span's window of
//                     rows by bisection, reads the target and tests its bit in the bitmap of U; one kept count per span
//   k_sub_write       the same span, the same flags, prefix-summed over the workgroup tile by tile: a kept edge writes the
//                     rank of its target and its place in the graph's col; the prefix sums stay in LDS, and every row whose
//                     scanned edges start in the span reads sub_ptr from them
// Work is cut by scanned edges, not by rows: a hub's row is as many spans as it is long, and a span that lies inside one row
// bisects nothing.  Integers only.  The scans are three launches each on purpose: no workgroup ever waits for another one --
// no look-back chain, no flags, no spinning -- and there are no atomics.  Every kernel strides over its work, so the grid is a
// matter of speed only; every store is inside the bounds its caller passes (a node of U outside [0, n) has no edges, an edge
// outside [0, nnz) or with a target outside [0, n) is not kept, a place outside the room of sub_col / sub_eid is not written).
// No scratch, nothing spilled.
#pragma once
#include "fora_kernels.h" // BLOCK, block_excl_scan, block_excl_scan64
#include "fora_subgraph_plan.h"

namespace fora {

// the out-degree of U[j], and where its row starts in the graph's col
__device__ __forceinline__ uint64_t sub_row_deg(const int32_t *__restrict__ U, const int64_t *__restrict__ row_ptr, uint32_t n, uint64_t j, int64_t &first) {
    const uint32_t u = (uint32_t)U[j];
    if (u >= n) { first = 0; return 0; }
    first = row_ptr[u];
    const int64_t len = row_ptr[u + 1] - first;
    return len > 0 ? (uint64_t)len : 0;
}

// total[b] = the out-degrees of rows [b * BLOCK, (b + 1) * BLOCK) of U below nc
__global__ __launch_bounds__(BLOCK) void k_sub_row_totals(const int32_t *__restrict__ U, uint64_t nc, const int64_t *__restrict__ row_ptr, uint32_t n, uint64_t blocks,
                                                          uint64_t *__restrict__ total) {
    __shared__ uint64_t s_w[BLOCK / 64];
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint64_t j = b * BLOCK + threadIdx.x;
        int64_t first;
        const uint64_t deg = j < nc ? sub_row_deg(U, row_ptr, n, j, first) : 0;
        uint64_t tot;
        (void)block_excl_scan64(deg, s_w, tot);
        if (threadIdx.x == 0) total[b] = tot;
    }
}

// off[i] = in[0] + .. + in[i - 1]; *sum = the sum of all.  One workgroup: launched with a grid of one.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_sub_scan(const T *__restrict__ in, uint64_t count, uint64_t *__restrict__ off, unsigned long long *sum) {
    __shared__ uint64_t s_w[BLOCK / 64];
    if (blockIdx.x) return;
    uint64_t carry = 0;
    for (uint64_t i0 = 0; i0 < count; i0 += BLOCK) { // (more totals than threads: the loop)
        const uint64_t i = i0 + threadIdx.x;
        const uint64_t t = i < count ? (uint64_t)in[i] : 0;
        uint64_t tot;
        const uint64_t x = block_excl_scan64(t, s_w, tot);
        if (i < count) off[i] = carry + x;
        carry += tot;
    }
    if (threadIdx.x == 0) *sum = carry;
}

// scan_ptr[j] = off[j / BLOCK] + the out-degrees of the block's rows in front of j; base[j] = row_ptr[U[j]] - scan_ptr[j];
// the last row writes scan_ptr[nc] on top
__global__ __launch_bounds__(BLOCK) void k_sub_row_list(const int32_t *__restrict__ U, uint64_t nc, const int64_t *__restrict__ row_ptr, uint32_t n, uint64_t blocks,
                                                        const uint64_t *__restrict__ off, int64_t *__restrict__ scan_ptr, int64_t *__restrict__ base) {
    __shared__ uint64_t s_w[BLOCK / 64];
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint64_t j = b * BLOCK + threadIdx.x;
        int64_t first = 0;
        const uint64_t deg = j < nc ? sub_row_deg(U, row_ptr, n, j, first) : 0;
        uint64_t tot;
        const uint64_t at = off[b] + block_excl_scan64(deg, s_w, tot);
        if (j >= nc) continue;
        scan_ptr[j] = (int64_t)at;
        base[j] = first - (int64_t)at;
        if (j + 1 == nc) scan_ptr[nc] = (int64_t)(at + deg);
    }
}

// A span of the scanned edges: [start, start + len) and the window of rows lo .. hi its edges lie in
struct SubSpan { int64_t start; uint32_t len; int64_t lo, hi; };
__device__ __forceinline__ SubSpan sub_span_of(const int64_t *__restrict__ scan_ptr, uint64_t nc, uint64_t S, uint32_t span, uint64_t s) {
    SubSpan w;
    w.start = (int64_t)(s * span);
    const uint64_t left = S - (uint64_t)w.start;
    w.len = left < span ? (uint32_t)left : span;
    const auto ptr = [&](int64_t i) { return scan_ptr[i]; };
    w.lo = sub_find_row(ptr, 0, (int64_t)nc - 1, w.start);
    w.hi = sub_find_row(ptr, w.lo, (int64_t)nc - 1, w.start + w.len - 1);
    return w;
}
// scanned edge p of a span: its place e in the graph's col, its target t, and whether it is kept (t in U)
__device__ __forceinline__ bool sub_edge(const SubSpan &w, int64_t p, const int64_t *__restrict__ scan_ptr, const int64_t *__restrict__ base,
                                         const int32_t *__restrict__ col, uint64_t nnz, const unsigned long long *__restrict__ bitmap, uint32_t n, int64_t &e, uint32_t &t) {
    const int64_t r = sub_find_row([&](int64_t i) { return scan_ptr[i]; }, w.lo, w.hi, p);
    e = base[r] + p;
    if ((uint64_t)e >= nnz) { t = n; return false; }
    t = (uint32_t)col[e];
    return t < n && sub_member(bitmap[cols_word_of(t)], t);
}

// cnt[s] = the kept edges of span s
__global__ __launch_bounds__(BLOCK) void k_sub_count(const int64_t *__restrict__ scan_ptr, const int64_t *__restrict__ base, uint64_t nc, uint64_t S, uint32_t span, uint64_t spans,
                                                     const int32_t *__restrict__ col, uint64_t nnz, const unsigned long long *__restrict__ bitmap, uint32_t n,
                                                     uint32_t *__restrict__ cnt) {
    __shared__ uint32_t s_w[BLOCK / 64];
    for (uint64_t s = blockIdx.x; s < spans; s += gridDim.x) {
        const SubSpan w = sub_span_of(scan_ptr, nc, S, span, s);
        uint32_t kept = 0;
        for (uint32_t i = threadIdx.x; i < w.len; i += BLOCK) {
            int64_t e; uint32_t t;
            kept += sub_edge(w, w.start + i, scan_ptr, base, col, nnz, bitmap, n, e, t) ? 1u : 0u;
        }
        uint32_t tot;
        (void)block_excl_scan(kept, s_w, tot);
        if (threadIdx.x == 0) cnt[s] = tot;
    }
}

// The kept edges of span s go to sub_col / sub_eid from off[s] on (room: cap entries); sub_ptr[j] for every row j of U whose
// scanned edges start in the span (the last span: at S too, and sub_ptr[nc]).  Dynamic LDS: span + 1 words.
__global__ __launch_bounds__(BLOCK) void k_sub_write(const int64_t *__restrict__ scan_ptr, const int64_t *__restrict__ base, uint64_t nc, uint64_t S, uint32_t span, uint64_t spans,
                                                     const int32_t *__restrict__ col, uint64_t nnz, const unsigned long long *__restrict__ bitmap,
                                                     const uint32_t *__restrict__ wrank, uint32_t n, const uint64_t *__restrict__ off,
                                                     int64_t *__restrict__ sub_ptr, int32_t *__restrict__ sub_col, int64_t *__restrict__ sub_eid, uint64_t cap) {
    extern __shared__ uint32_t sub_pref[]; // [span + 1] the kept edges of the span in front of each of its edges; [len]: all of them
    __shared__ uint32_t s_w[BLOCK / 64];
    for (uint64_t s = blockIdx.x; s < spans; s += gridDim.x) {
        const SubSpan w = sub_span_of(scan_ptr, nc, S, span, s);
        const uint64_t first = off[s];
        uint32_t carry = 0;
        for (uint32_t i0 = 0; i0 < w.len; i0 += BLOCK) { // (uniform bounds: every thread meets the scan's barriers)
            const uint32_t i = i0 + threadIdx.x;
            int64_t e = 0; uint32_t t = n;
            const bool keep = i < w.len && sub_edge(w, w.start + i, scan_ptr, base, col, nnz, bitmap, n, e, t);
            uint32_t tot;
            const uint32_t x = carry + block_excl_scan(keep ? 1u : 0u, s_w, tot);
            carry += tot;
            if (i < w.len) sub_pref[i] = x;
            const uint64_t k = first + x;
            if (keep && k < cap) {
                const uint64_t word = cols_word_of(t);
                sub_col[k] = (int32_t)cols_rank(wrank[word], bitmap[word], t & 63);
                sub_eid[k] = e;
            }
        }
        if (threadIdx.x == 0) sub_pref[w.len] = carry;
        __syncthreads();
        const auto ptr = [&](int64_t i) { return scan_ptr[i]; };
        const int64_t ja = sub_rows_from(ptr, (int64_t)nc, w.start);
        const int64_t jb = s + 1 == spans ? (int64_t)nc + 1 : sub_rows_from(ptr, (int64_t)nc, w.start + w.len);
        for (int64_t j = ja + threadIdx.x; j < jb; j += BLOCK) {
            const uint64_t at = (uint64_t)(scan_ptr[j] - w.start);
            if ((uint64_t)j <= nc && at <= w.len) sub_ptr[j] = (int64_t)(first + sub_pref[at]);
        }
        __syncthreads(); // (the next span of this workgroup writes sub_pref again)
    }
}

} // namespace fora
