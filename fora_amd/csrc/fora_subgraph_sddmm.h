// fora_subgraph_sddmm.h -- the kernel of EDGE SCORES (fora_hip_subgraph_sddmm; the contract is in include/fora_hip_edge.h): for
// every edge e of row j of the held subgraph with target v = sub_col[e], and every head h,
//   score[h][e] = <a[j][h*d .. (h+1)*d), b[v][h*d .. (h+1)*d)>
// under the SCORES (SDDMM) contract of fora_sddmm.h applied to the head's column slice: exact f64 products, the 64 running sums
// q_l over c == l (mod 64) in ascending c from +0.0, the tree o = 32 .. 1.
// The work is cut by EDGES, not by rows, and nothing is planned on the host: a wave owns SUBS_SPAN = 64 consecutive places of
// sub_col -- a hub's row is as many waves as it is long, a run of three-edge rows fills one -- and finds its rows itself:
//   1. the row j0 of its first edge by bisection over sub_ptr (wave-uniform: scalar loads);
//   2. the rows of the other edges by walking sub_ptr from j0 + 1, 64 rows a step: a NON-EMPTY row that starts inside the span
//      writes its number at the place of its first edge in the wave's 64 words of LDS (one writer per word: of the rows that
//      start at one place only the last is not empty), and a running maximum over the lanes hands every edge the last row that
//      started at or before it.  Empty rows -- leading, trailing, in runs -- write nothing and are stepped over.
// The items of a wave are the (edge, head) pairs of its edges, p = k * heads + h.  A group of G lanes (fora_sddmm.h) owns a
// pair, SDDMM_INFLIGHT = 4 of them per round, whose four trees share their first two exchanges exactly as in sddmm_scores;
// groups side by side hold consecutive heads of one edge, so they read side-by-side slices of ONE row of b -- the row comes
// in once, as whole lines, for all heads -- and of one row of a, whose re-reads by the edge's later pairs and by the row's
// later edges are cache hits.  The lane that ends with a pair's score stores it to out[h * edges + e].
// No bit depends on the grid, on heads being one call or many, or on anything else here.  Integers and LDS hold rows only;
// the sums live in registers.  Compiled with -ffp-contract=off, and the kernel says so again itself.
#pragma once
#include "fora_attn.h"  // attn_wave_sync
#include "fora_sddmm.h" // sddmm_load, sddmm_types, SDDMM_INFLIGHT

namespace fora {

constexpr uint32_t SUBS_SPAN = 64;          // edges of sub_col one wave scores: one per lane while it finds their rows
constexpr uint32_t SUBS_WAVES = BLOCK / 64; // spans per workgroup and step
static_assert(SUBS_SPAN == 64, "a lane per edge of the span");

// grid = ceil(spans / SUBS_WAVES) workgroups of BLOCK threads: wave w of the grid takes span w.  lg = log2(G), G the group of d columns.
template <int A_ET, int B_ET>
__global__ void __launch_bounds__(BLOCK) k_sub_sddmm(const int64_t *__restrict__ sub_ptr, uint32_t nc, const int32_t *__restrict__ sub_col, uint64_t edges,
                                                     const void *a, int64_t lda, const void *b, int64_t ldb, uint32_t d, uint32_t heads, uint32_t lg,
                                                     float *out32, double *out64, uint32_t types) {
#pragma clang fp contract(off)
    __shared__ uint32_t sh_row[SUBS_WAVES][SUBS_SPAN];
    const int a_rt = (int)(types & 0xFFu), b_rt = (int)(types >> 8);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // (uniform, and the compiler knows it)
    uint32_t *rows = sh_row[wave];
    const uint32_t G = 1u << lg;
    const uint32_t gl = lane & (G - 1u), grp = lane >> lg, ngrp = 64u >> lg;
    {
        const uint64_t e0 = ((uint64_t)blockIdx.x * SUBS_WAVES + wave) * SUBS_SPAN;
        if (e0 >= edges) return; // (the whole wave; there is no workgroup barrier below)
        const uint32_t cnt = (uint32_t)min((uint64_t)SUBS_SPAN, edges - e0);
        const int64_t e_end = (int64_t)(e0 + cnt);
        // ---- 1. j0: the last row that starts at or before e0 -- it holds e0, since sub_ptr[j0 + 1] > e0.  sub_ptr[0] = 0 <= e0 < edges = sub_ptr[nc].
        uint32_t j0 = 0, hi = nc;
        while (hi - j0 > 1u) {
            const uint32_t mid = j0 + ((hi - j0) >> 1);
            if (sub_ptr[mid] <= (int64_t)e0) j0 = mid; else hi = mid;
        }
        // ---- 2. the rows that start inside (e0, e_end), from j0 + 1 on
        rows[lane] = j0;
        attn_wave_sync();
        for (uint64_t r0 = (uint64_t)j0 + 1;; r0 += 64) {
            const uint64_t r = r0 + lane;
            int64_t first = INT64_MAX, next = INT64_MAX; // (past the last row: nothing starts there)
            if (r < nc) { first = sub_ptr[r]; next = sub_ptr[r + 1]; }
            if (first < e_end && next > first) rows[(uint32_t)(first - (int64_t)e0)] = (uint32_t)r; // (first > e0: r > j0)
            if (__shfl(next, 63) >= e_end) break; // (uniform: every later row starts behind the span)
        }
        attn_wave_sync();
        uint32_t row = rows[lane];
#pragma unroll
        for (uint32_t o = 1; o < 64u; o <<= 1) {
            const uint32_t t = __shfl_up(row, o);
            if (lane >= o) row = max(row, t);
        }
        attn_wave_sync(); // (every lane has read its word)
        rows[lane] = row;
        attn_wave_sync();
        // ---- 3. the pairs (edge k, head h) of the span, p = k * heads + h: group g takes p0 + g, p0 + ngrp + g, ...
        const uint32_t np = cnt * heads; // (at most 64 * 65536)
        for (uint32_t p0 = 0; p0 < np; p0 += ngrp * SDDMM_INFLIGHT) {
            uint64_t arow[SDDMM_INFLIGHT], brow[SDDMM_INFLIGHT], at[SDDMM_INFLIGHT];
            bool valid[SDDMM_INFLIGHT];
            double q[SDDMM_INFLIGHT];
#pragma unroll
            for (int u = 0; u < SDDMM_INFLIGHT; u++) {
                const uint32_t p = p0 + (uint32_t)u * ngrp + grp;
                valid[u] = p < np;
                // a pair past the count is scored as pair 0 again -- memory the wave reads anyway, no branch around a load -- and never stored
                const uint32_t k = valid[u] ? (heads == 1u ? p : p / heads) : 0u; // (k < cnt: a place of rows that was written)
                const uint32_t h = valid[u] ? p - k * heads : 0u;
                const uint64_t col0 = (uint64_t)h * d;
                arow[u] = (uint64_t)rows[k] * (uint64_t)lda + col0;
                brow[u] = (uint64_t)(uint32_t)sub_col[e0 + k] * (uint64_t)ldb + col0;
                at[u] = (uint64_t)h * edges + e0 + k;
                q[u] = 0.0;
            }
            for (uint32_t c = gl; c < d; c += 64u) {
                uint32_t ra[SDDMM_INFLIGHT], rb[SDDMM_INFLIGHT];
#pragma unroll
                for (int u = 0; u < SDDMM_INFLIGHT; u++) {
                    ra[u] = sddmm_load<A_ET>(a, arow[u] + c, a_rt);
                    rb[u] = sddmm_load<B_ET>(b, brow[u] + c, b_rt);
                }
#pragma unroll
                for (int u = 0; u < SDDMM_INFLIGHT; u++) {
                    const double t = (double)__uint_as_float(ra[u]) * (double)__uint_as_float(rb[u]);
                    q[u] = q[u] + t;
                }
            }
            if (G >= 4u) {
                // the four trees of the round share their first two exchanges: sddmm_scores says why the bits are the contract's
                const uint32_t o1 = G >> 1, o2 = G >> 2;
                const bool up1 = (gl & o1) != 0, up2 = (gl & o2) != 0;
                const double r0 = (up1 ? q[1] : q[0]) + __shfl_xor(up1 ? q[0] : q[1], (int)o1, (int)G);
                const double r1 = (up1 ? q[3] : q[2]) + __shfl_xor(up1 ? q[2] : q[3], (int)o1, (int)G);
                double s = (up2 ? r1 : r0) + __shfl_xor(up2 ? r0 : r1, (int)o2, (int)G);
                for (uint32_t o = G >> 3; o; o >>= 1) s = s + __shfl_xor(s, (int)o, (int)G);
                if ((gl & (o2 - 1u)) == 0) { // the first lane of a quarter holds pair (2 if the second quarter of its half) + (1 if the upper half)
                    const bool ok = up2 ? (up1 ? valid[3] : valid[2]) : (up1 ? valid[1] : valid[0]);
                    const uint64_t o = up2 ? (up1 ? at[3] : at[2]) : (up1 ? at[1] : at[0]);
                    if (ok) {
                        if (out64) out64[o] = s;
                        if (out32) out32[o] = (float)s;
                    }
                }
            } else {
                if (G == 2u) {
#pragma unroll
                    for (int u = 0; u < SDDMM_INFLIGHT; u++) q[u] = q[u] + __shfl_down(q[u], 1u, 2);
                }
                if (gl == 0) {
#pragma unroll
                    for (int u = 0; u < SDDMM_INFLIGHT; u++) {
                        if (!valid[u]) continue;
                        if (out64) out64[at[u]] = q[u];
                        if (out32) out32[at[u]] = (float)q[u];
                    }
                }
            }
        }
    }
}

} // namespace fora
