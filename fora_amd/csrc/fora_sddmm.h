// fora_sddmm.h -- the kernel of SCORES (SDDMM) (fora_hip_sparse_sddmm; the contract is in include/fora_hip.h): for every
// held entry e of row i with id v, score_e = <A[i], B[v]> over d columns, every bit defined.
//   t_c   = (double)A[i][c] * (double)B[v][c] -- exact: two 24-bit significands, and the exponents fit;
//   q_l   = the t_c with c == l (mod 64) added in ascending c from +0.0, l = 0 .. 63;
//   tree  for o = 32, 16, 8, 4, 2, 1: q_l = q_l + q_{l+o} for l < o;  score_e = q_0.
// A group of G lanes (a power of two, the smallest that holds d, at most 64) owns an entry: lane l holds q_l.  With G < 64
// the q_l of l >= G are +0.0 and no q_l is ever -0.0, so the steps o >= G of the tree change no bit and the group runs only
// its own.  The work list is the segment list of fora_prop_plan.h; a wave takes SDDMM_SUB entries of one segment -- one row
// of A, re-read per column block from the cache -- and every group has the B rows of SDDMM_INFLIGHT entries in flight, whose
// four trees share their first two exchanges (below).  The loop over a wave's entries is sddmm_scores, which the fused
// attention kernel (fora_attn.h) calls too: what becomes of a finished score is the caller's.
// Nothing is fused: the file is compiled with -ffp-contract=off and the kernel says so again itself.
#pragma once
#include "fora_kernels.h" // BLOCK
#include "fora_narrow.h" // the element types, narrow_widen
#include "fora_prop_plan.h"

namespace fora {

constexpr uint32_t SDDMM_SUB = 64;     // entries of a segment that one wave scores
constexpr uint32_t SDDMM_UNITS = PROP_SEG / SDDMM_SUB; // waves per segment
constexpr int SDDMM_INFLIGHT = 4;      // entries a lane group has in flight
static_assert(SDDMM_INFLIGHT == 4, "k_prop_sddmm merges the trees of exactly four entries");

// One element as the bits of its f32 widening.  ET: the element type where the kernel was compiled for it -- f32 and bf16, the
// two that the instantiations of old take -- or ELT_ANY: the type is rt, the same for the whole wave, and the load switches on
// it (one element per lane: nothing about the lanes' layout hangs on the type, and a class of its own for every pair of
// five types would be 25 kernels where there are 5).
template <int ET> __device__ __forceinline__ uint32_t sddmm_load(const void *m, uint64_t at, int rt) {
    static_assert(ET == ELT_F32 || ET == ELT_BF16 || ET == ELT_ANY, "a compiled-in type is f32 or bf16");
    if constexpr (ET == ELT_BF16) return (uint32_t)((const uint16_t *)m)[at] << 16;
    else if constexpr (ET == ELT_F32) return __float_as_uint(((const float *)m)[at]);
    else {
        switch (rt) {
        case ELT_F32: return __float_as_uint(((const float *)m)[at]);
        case ELT_BF16: return (uint32_t)((const uint16_t *)m)[at] << 16;
        case ELT_F16: return __float_as_uint(narrow_widen<ELT_F16>(((const uint16_t *)m)[at]));
        case ELT_E4M3: return __float_as_uint(narrow_widen<ELT_E4M3>(((const uint8_t *)m)[at]));
        default: return __float_as_uint(narrow_widen<ELT_E5M2>(((const uint8_t *)m)[at]));
        }
    }
}
// the run-time types of a and b in one kernel argument (read only by the ELT_ANY instantiations)
constexpr uint32_t sddmm_types(int a_type, int b_type) { return (uint32_t)a_type | (uint32_t)b_type << 8; }

// The scores of `cnt` entries with the ids ids[0 .. cnt) against one row of a (arow: its first element), by one whole wave;
// lg = log2(G).  Group g of the wave's 64 / G groups takes the entries g, g + 64 / G, ..., SDDMM_INFLIGHT of them per round.
// Every lane of the wave runs every round (the shuffles of the tree want whole groups); an entry past the count loads nothing
// and is never handed on.  bcol: the first column of b that counts (a column slice: a head), added to every row's place.
// sink(k, s): called once per entry k < cnt, on the lane that ends up with its score s -- the one thing in which the callers
// differ (k_prop_sddmm stores it, k_attn_short of fora_attn.h keeps it in LDS).
// A_ET, B_ET: the element types of a and b as sddmm_load takes them; types: sddmm_types() of the two, for ELT_ANY.
template <int A_ET, int B_ET, typename Sink>
__device__ __forceinline__ void sddmm_scores(const int32_t *ids, uint32_t cnt, const void *a, uint64_t arow, const void *b, int64_t ldb, uint64_t bcol,
                                             uint32_t d, uint32_t lg, uint32_t lane, uint32_t types, Sink &&sink) {
#pragma clang fp contract(off)
    const int a_rt = (int)(types & 0xFFu), b_rt = (int)(types >> 8);
    const uint32_t G = 1u << lg;
    const uint32_t gl = lane & (G - 1u), grp = lane >> lg, ngrp = 64u >> lg;
    for (uint32_t j0 = 0; j0 < cnt; j0 += ngrp * SDDMM_INFLIGHT) {
        uint64_t brow[SDDMM_INFLIGHT];
        bool valid[SDDMM_INFLIGHT];
        double q[SDDMM_INFLIGHT];
#pragma unroll
        for (int u = 0; u < SDDMM_INFLIGHT; u++) {
            const uint32_t k = j0 + (uint32_t)u * ngrp + grp;
            valid[u] = k < cnt;
            brow[u] = valid[u] ? (uint64_t)(uint32_t)ids[k] * (uint64_t)ldb + bcol : 0ull;
            q[u] = 0.0;
        }
        for (uint32_t c = gl; c < d; c += 64u) {
            const double av = (double)__uint_as_float(sddmm_load<A_ET>(a, arow + c, a_rt));
            uint32_t raw[SDDMM_INFLIGHT];
#pragma unroll
            for (int u = 0; u < SDDMM_INFLIGHT; u++) raw[u] = valid[u] ? sddmm_load<B_ET>(b, brow[u] + c, b_rt) : 0u;
#pragma unroll
            for (int u = 0; u < SDDMM_INFLIGHT; u++) {
                const double t = av * (double)__uint_as_float(raw[u]);
                q[u] = q[u] + t;
            }
        }
        if (G >= 4u) {
            // the four trees of the round share their shuffles.  Step o = G / 2: the lower half of the group goes on with
            // entry 0 (2) and the upper half with entry 1 (3) -- a lane sends its partner the q of the entry the partner keeps,
            // so one exchange serves two entries.  Step o = G / 4 does the same with the two results.  From there a quarter of
            // the group holds one entry's q_0 .. q_{G/4-1} and the rest of the tree is a butterfly inside the quarter.  An add
            // gives the same bits whichever operand comes first, so lane l of an upper half, which adds q_{l'+o} + q_{l'} for
            // l' = l - o, computes the contract's q_{l'} + q_{l'+o}.
            const uint32_t o1 = G >> 1, o2 = G >> 2;
            const bool up1 = (gl & o1) != 0, up2 = (gl & o2) != 0;
            const double r0 = (up1 ? q[1] : q[0]) + __shfl_xor(up1 ? q[0] : q[1], (int)o1, (int)G);
            const double r1 = (up1 ? q[3] : q[2]) + __shfl_xor(up1 ? q[2] : q[3], (int)o1, (int)G);
            double s = (up2 ? r1 : r0) + __shfl_xor(up2 ? r0 : r1, (int)o2, (int)G);
            for (uint32_t o = G >> 3; o; o >>= 1) s = s + __shfl_xor(s, (int)o, (int)G);
            if ((gl & (o2 - 1u)) == 0) { // the first lane of a quarter: the entry (2 if the second quarter of its half) + (1 if the upper half)
                const uint32_t u = (up2 ? 2u : 0u) + (up1 ? 1u : 0u);
                const uint32_t k = j0 + u * ngrp + grp;
                if (k < cnt) sink(k, s);
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
                    sink(j0 + (uint32_t)u * ngrp + grp, q[u]);
                }
            }
        }
    }
}

// grid = ceil(nseg * SDDMM_UNITS / (BLOCK / 64)) workgroups of BLOCK threads; lg = log2(G).  Wave u of the grid owns the
// entries [sub * SDDMM_SUB, ...) of segment u / SDDMM_UNITS, sub = u % SDDMM_UNITS, and scores them with sddmm_scores.
template <int A_ET, int B_ET>
__global__ void __launch_bounds__(BLOCK) k_prop_sddmm(const PropSeg *segs, uint64_t nseg, const int32_t *ids, const void *a, int64_t lda, const void *b,
                                                      int64_t ldb, uint32_t d, uint32_t lg, float *out32, double *out64, uint32_t types) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t unit = (uint64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t s = unit / SDDMM_UNITS;
    const uint32_t lo = (uint32_t)(unit % SDDMM_UNITS) * SDDMM_SUB;
    if (s >= nseg) return; // (the whole wave)
    const PropSeg sg = segs[s];
    if (lo >= sg.len) return;
    const uint32_t cnt = min(SDDMM_SUB, sg.len - lo);
    const int64_t e0 = sg.first + lo;
    const uint64_t arow = (uint64_t)(uint32_t)sg.row * (uint64_t)lda;
    sddmm_scores<A_ET, B_ET>(ids + e0, cnt, a, arow, b, ldb, 0ull, d, lg, lane, types, [=](uint32_t k, double sc) {
        if (out64) out64[e0 + k] = sc;
        if (out32) out32[e0 + k] = (float)sc;
    });
}

} // namespace fora
