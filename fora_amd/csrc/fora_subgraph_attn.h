// fora_subgraph_attn.h -- the fused kernel of EDGE ATTENTION (fora_hip_subgraph_attention; the contract is in
// include/fora_hip_edge_attention.h): for a GROUP of at most PROP_SEG = 256 edges of the held subgraph -- a row j of sub_ptr, or
// by column the positions in_ptr[u] .. in_ptr[u + 1] of its transposition -- EDGE SCORES, EDGE SOFTMAX and the SUBGRAPH PRODUCT
// with values in one wave, nothing leaving the CU between the steps and every bit what the three calls chained through f64 give.
// The cut is not k_attn_short's (a wave per (row, head)): a group has a few dozen edges and dv is small in a GAT layer, so a wave
// owns one group and a CHUNK of up to SGA_HEADS = 4 consecutive heads, unit u = group u / chunks, chunk u % chunks:
//   staging  the group's feature-row ids -- sub_col[e] by row, in_row[p] by column -- once in the wave's LDS; the places of its
//            entries in sub_col (in_pos[p] by column) stay in registers, four a lane as in ssm_places: only the y stores need them.
//   scores   the items are the (edge, head) pairs of the chunk, p = k * hc + h, side by side as in step 3 of k_sub_sddmm: a lane
//            group per pair, four pairs in flight, the merged trees.  Groups side by side hold the chunk's heads of ONE edge, so a
//            row of k comes in once for the chunk, as whole lines.  The products are exact and commute, so <k[row], q[u]> by column
//            is the same bits as <q[u], k[row]>: both groupings read q at the group and k at the id.  A score goes to
//            ysh[h - h0][place in the group].
//   softmax  in registers with the functions of fora_softmax.h and fora_subgraph_softmax.h as they stand, the LDS array read as
//            the `scores` of a head: a group of at most 64 edges holds one value a lane with the chunk's heads in flight, a longer
//            one four values a lane, one head at a time.  y goes to the y outputs at h * edges + place, and back to LDS.
//   product  lanes span the chunk's contiguous columns [h0 * dv, (h0 + hc) * dv) of v, V adjacent per lane (the host chose V by
//            attn_vec_width, so a lane's columns lie in one head); a lane's weight for entry e is ysh[head of its columns][e];
//            the entries one after the other in group order from +0.0, PROP_INFLIGHT rows of v in flight.  A row of v is read
//            once for all heads of the chunk.
// A NaN (group, head) is wave-uniform per head: the quiet NaN is selected into its y and its dv stores, lane 0 counts it.  An
// empty group writes +0.0; a group longer than the cap leaves (the host runs it through the three steps' own kernels).
// A wave's LDS is its own -- SGA_HEADS x 256 doubles and 256 ids, 9 KB -- and what one lane writes another reads only behind
// attn_wave_sync: no workgroup barrier.  Compiled with -ffp-contract=off, and the kernel says so again itself.
#pragma once
#include "fora_attn.h"             // attn_wave_sync, PropRaw and the loads of fora_prop.h
#include "fora_sddmm.h"            // sddmm_load, SDDMM_INFLIGHT
#include "fora_subgraph_softmax.h" // ssm_places, ssm_load_x, ssm_exp_q, ssm_store, ssm_head

namespace fora {

constexpr uint32_t SGA_WAVES = BLOCK / 64; // units per workgroup, one wave each
constexpr int SGA_HEADS = 4;               // heads of a chunk: the rows of a wave's score array
static_assert(SGA_HEADS <= 32, "a chunk's NaN heads are the bits of one word");

// the chunk's scores: pair p = k * hc + h of entry k and head h0 + h to ysh[h * PROP_SEG + k].  qrow: the first element of the
// group's row of q, col0 = h0 * d.  Every lane runs every round; a pair past the count is scored as pair 0 again and dropped.
template <int Q_ET, int K_ET>
__device__ __forceinline__ void sga_scores(const int32_t *idsh, uint32_t len, uint32_t hc, const void *q, uint64_t qrow, const void *k, int64_t ldk, uint64_t col0,
                                           uint32_t d, uint32_t lg, uint32_t lane, uint32_t types, double *ysh) {
#pragma clang fp contract(off)
    const int q_rt = (int)(types & 0xFFu), k_rt = (int)(types >> 8);
    const uint32_t G = 1u << lg;
    const uint32_t gl = lane & (G - 1u), grp = lane >> lg, ngrp = 64u >> lg;
    const uint32_t np = len * hc; // (at most 256 * SGA_HEADS)
    for (uint32_t p0 = 0; p0 < np; p0 += ngrp * SDDMM_INFLIGHT) {
        uint64_t qat[SDDMM_INFLIGHT], kat[SDDMM_INFLIGHT];
        uint32_t slot[SDDMM_INFLIGHT];
        bool valid[SDDMM_INFLIGHT];
        double s[SDDMM_INFLIGHT];
#pragma unroll
        for (int u = 0; u < SDDMM_INFLIGHT; u++) {
            const uint32_t p = p0 + (uint32_t)u * ngrp + grp;
            valid[u] = p < np;
            const uint32_t e = valid[u] ? (hc == 1u ? p : p / hc) : 0u;
            const uint32_t h = valid[u] ? p - e * hc : 0u;
            const uint64_t col = col0 + (uint64_t)h * d;
            qat[u] = qrow + col;
            kat[u] = (uint64_t)(uint32_t)idsh[e] * (uint64_t)ldk + col;
            slot[u] = h * PROP_SEG + e;
            s[u] = 0.0;
        }
        for (uint32_t c = gl; c < d; c += 64u) {
            uint32_t rq[SDDMM_INFLIGHT], rk[SDDMM_INFLIGHT];
#pragma unroll
            for (int u = 0; u < SDDMM_INFLIGHT; u++) {
                rq[u] = sddmm_load<Q_ET>(q, qat[u] + c, q_rt);
                rk[u] = sddmm_load<K_ET>(k, kat[u] + c, k_rt);
            }
#pragma unroll
            for (int u = 0; u < SDDMM_INFLIGHT; u++) {
                const double t = (double)__uint_as_float(rq[u]) * (double)__uint_as_float(rk[u]);
                s[u] = s[u] + t;
            }
        }
        if (G >= 4u) {
            // the four trees of the round share their first two exchanges: sddmm_scores says why the bits are the contract's
            const uint32_t o1 = G >> 1, o2 = G >> 2;
            const bool up1 = (gl & o1) != 0, up2 = (gl & o2) != 0;
            const double r0 = (up1 ? s[1] : s[0]) + __shfl_xor(up1 ? s[0] : s[1], (int)o1, (int)G);
            const double r1 = (up1 ? s[3] : s[2]) + __shfl_xor(up1 ? s[2] : s[3], (int)o1, (int)G);
            double t = (up2 ? r1 : r0) + __shfl_xor(up2 ? r0 : r1, (int)o2, (int)G);
            for (uint32_t o = G >> 3; o; o >>= 1) t = t + __shfl_xor(t, (int)o, (int)G);
            if ((gl & (o2 - 1u)) == 0) { // the first lane of a quarter holds pair (2 if the second quarter of its half) + (1 if the upper half)
                const bool ok = up2 ? (up1 ? valid[3] : valid[2]) : (up1 ? valid[1] : valid[0]);
                const uint32_t at = up2 ? (up1 ? slot[3] : slot[2]) : (up1 ? slot[1] : slot[0]);
                if (ok) ysh[at] = t;
            }
        } else {
            if (G == 2u) {
#pragma unroll
                for (int u = 0; u < SDDMM_INFLIGHT; u++) s[u] = s[u] + __shfl_down(s[u], 1u, 2);
            }
            if (gl == 0) {
#pragma unroll
                for (int u = 0; u < SDDMM_INFLIGHT; u++)
                    if (valid[u]) ysh[slot[u]] = s[u];
            }
        }
    }
}

// the softmax of the chunk's heads, U of them in flight with PER values a lane each: a lane reads the scores at its own
// places lane + 64 j of a head's row of ysh and writes y there again -- no lane touches another's -- and to the y outputs
// at the entries' places `at`.  A head past the chunk is its last head again, never stored or counted.  Returns the chunk's
// NaN heads, bit h - h0 (wave-uniform).
template <int PER, int U>
__device__ __forceinline__ uint32_t sga_softmax(double *ysh, const uint64_t (&at)[PER], uint32_t len, uint32_t lane, uint32_t h0, uint32_t hc, uint64_t edges,
                                                double scale, float *y32, double *y64) {
#pragma clang fp contract(off)
    uint64_t self[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) self[j] = lane + 64u * (uint32_t)j;
    uint32_t nan_heads = 0;
    for (uint32_t b = 0; b < hc; b += (uint32_t)U) {
        double x[U][PER], m[U], q[U];
        uint32_t h[U];
        bool bad[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            h[u] = min(b + (uint32_t)u, hc - 1u);
            m[u] = ssm_load_x<double, PER>(self, len, lane, ysh + h[u] * PROP_SEG, scale, x[u]);
        }
#pragma unroll
        for (int u = 0; u < U; u++) m[u] = smax_wave_max(m[u]);
#pragma unroll
        for (int u = 0; u < U; u++) {
            bad[u] = smax_is_inf(m[u]); // (the whole wave: a NaN entry, +inf, or nothing above -inf)
            q[u] = ssm_exp_q<PER>(len, lane, m[u], bad[u], x[u]);
        }
#pragma unroll
        for (int u = 0; u < U; u++) q[u] = smax_tree(q[u]);
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (b + (uint32_t)u >= hc) break;
#pragma unroll
            for (int j = 0; j < PER; j++) x[u][j] = bad[u] ? smax_nan() : x[u][j] / q[u];
            const uint64_t off = (uint64_t)(h0 + h[u]) * edges;
            ssm_store<PER>(at, len, lane, x[u], ssm_head(y32, off), ssm_head(y64, off));
            ssm_store<PER>(self, len, lane, x[u], nullptr, ysh + h[u] * PROP_SEG);
            nan_heads |= bad[u] ? 1u << h[u] : 0u;
        }
    }
    return nan_heads;
}

// the product of the chunk: wc = hc * dv columns from column vcol = h0 * dv of v; o32 / o64 point at the chunk's first output
// column of the group's row (either may be null).  attn_product with the weight of a lane taken from the head of its columns.
template <int ET, int V>
__device__ __forceinline__ void sga_product(const double *ysh, const int32_t *idsh, uint32_t len, const void *v, int64_t ldv, uint64_t vcol, uint32_t wc, uint32_t dv,
                                            uint32_t nan_heads, uint32_t lane, float *o32, double *o64) {
#pragma clang fp contract(off)
    for (uint32_t c0 = lane * (uint32_t)V; c0 < wc; c0 += 64u * (uint32_t)V) {
        const uint32_t ncol = min((uint32_t)V, wc - c0);
        const uint32_t hd = c0 / dv; // (V divides dv when there is more than one head: the lane's columns are this head's)
        const double *const yw = ysh + hd * PROP_SEG;
        double acc[V];
#pragma unroll
        for (int i = 0; i < V; i++) acc[i] = 0.0;
        for (uint32_t k = 0; k < len; k += PROP_INFLIGHT) {
            PropRaw<ET, V> raw[PROP_INFLIGHT];
            uint64_t off[PROP_INFLIGHT];
            double w[PROP_INFLIGHT];
#pragma unroll
            for (int u = 0; u < PROP_INFLIGHT; u++) {
                const uint32_t from = min(k + (uint32_t)u, len - 1u);
                off[u] = (uint64_t)(uint32_t)idsh[from] * (uint64_t)ldv + vcol + c0;
                w[u] = yw[from];
#pragma unroll
                for (int j = 0; j < PropRaw<ET, V>::W; j++) raw[u].w[j] = 0;
            }
            if (ncol == (uint32_t)V) { // (as in attn_product: the choice stands outside the loop over the rows)
#pragma unroll
                for (int u = 0; u < PROP_INFLIGHT; u++)
                    if (k + (uint32_t)u < len) prop_load_full<ET, V>(v, off[u], raw[u]);
            } else {
#pragma unroll
                for (int u = 0; u < PROP_INFLIGHT; u++)
                    if (k + (uint32_t)u < len) prop_load_tail<ET, V>(v, off[u], ncol, raw[u]);
            }
#pragma unroll
            for (int u = 0; u < PROP_INFLIGHT; u++) {
                const bool valid = k + (uint32_t)u < len;
#pragma unroll
                for (int i = 0; i < V; i++) {
                    const double term = w[u] * prop_widen<ET, V>(raw[u], i);
                    const double sum = acc[i] + term;
                    acc[i] = valid ? sum : acc[i];
                }
            }
        }
        const bool bad = (nan_heads >> hd & 1u) != 0; // a NaN (group, head) is written, not computed
#pragma unroll
        for (int i = 0; i < V; i++) {
            if ((uint32_t)i < ncol) {
                const double r = bad ? smax_nan() : acc[i];
                if (o64) o64[c0 + (uint32_t)i] = r;
                if (o32) o32[c0 + (uint32_t)i] = (float)r;
            }
        }
    }
}

// grid = ceil(ngroups * chunks / SGA_WAVES) workgroups of BLOCK threads, chunks = ceil(heads / SGA_HEADS).  ptr / ids / pos:
// sub_ptr, sub_col and null by row; in_ptr, in_row and in_pos by column.  q, k, v: the whole operands; head h reads the columns
// [h * d, (h + 1) * d) of q and k and [h * dv, (h + 1) * dv) of v.  lg = log2 of the lane group of the scores.  out32 / out64:
// ngroups x heads * dv with their own pitches, either may be null; y32 / y64: [heads][edges], both may be null.  Q_ET, K_ET: the
// types of q and k as sddmm_load takes them (types: sddmm_types() of the two, for ELT_ANY); V_ET: v's own type.
template <int Q_ET, int K_ET, int V_ET, int V, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_attn(const int64_t *__restrict__ ptr, uint32_t ngroups, uint32_t cap, const int32_t *__restrict__ ids,
                                                    const int64_t *__restrict__ pos, uint32_t heads, uint32_t chunks, const void *q, int64_t ldq, const void *k,
                                                    int64_t ldk, const void *v, int64_t ldv, uint32_t d, uint32_t dv, uint32_t lg, double scale, uint64_t edges,
                                                    float *out32, int64_t ld32, double *out64, int64_t ld64, float *y32, double *y64, uint32_t *nan_pairs,
                                                    uint32_t types) {
#pragma clang fp contract(off)
    __shared__ double sh_y[SGA_WAVES][SGA_HEADS * PROP_SEG];
    __shared__ int32_t sh_id[SGA_WAVES][PROP_SEG];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // (uniform, and the compiler knows it)
    const uint64_t u = (uint64_t)blockIdx.x * SGA_WAVES + wave;
    const uint64_t grp = u / chunks;
    if (grp >= ngroups) return; // (the whole wave; there is no workgroup barrier below)
    const uint32_t h0 = (uint32_t)(u % chunks) * (uint32_t)SGA_HEADS, hc = min((uint32_t)SGA_HEADS, heads - h0);
    const int64_t first = ptr[grp], count = ptr[grp + 1] - first; // (scalar loads)
    if (count > (int64_t)cap) return;                             // (the long path's)
    const uint32_t wc = hc * dv;
    float *const o32 = out32 ? out32 + (int64_t)grp * ld32 + (uint64_t)h0 * dv : nullptr;
    double *const o64 = out64 ? out64 + (int64_t)grp * ld64 + (uint64_t)h0 * dv : nullptr;
    if (count <= 0) { // an empty group: +0.0, whatever the cap
        for (uint32_t c = lane; c < wc; c += 64u) {
            if (o64) o64[c] = 0.0;
            if (o32) o32[c] = 0.0f;
        }
        return;
    }
    const uint32_t len = (uint32_t)count; // (at most PROP_SEG: the host clamps the cap)
    double *const ysh = sh_y[wave];
    int32_t *const idsh = sh_id[wave];
    uint64_t at[SMAX_PER_LANE];
    ssm_places<BYCOL, (int)SMAX_PER_LANE>(pos, first, len, lane, at);
#pragma unroll
    for (uint32_t j = 0; j < SMAX_PER_LANE; j++)
        if (lane + 64u * j < len) idsh[lane + 64u * j] = ids[first + lane + 64u * j];
    attn_wave_sync();
    sga_scores<Q_ET, K_ET>(idsh, len, hc, q, grp * (uint64_t)ldq, k, ldk, (uint64_t)h0 * d, d, lg, lane, types, ysh);
    attn_wave_sync();
    uint32_t nan_heads;
    if (len <= 64u) { // (uniform) a lane holds one value of a head, the chunk's heads interleave
        const uint64_t at1[1] = {at[0]};
        nan_heads = sga_softmax<1, SGA_HEADS>(ysh, at1, len, lane, h0, hc, edges, scale, y32, y64);
    } else {
        nan_heads = sga_softmax<(int)SMAX_PER_LANE, 1>(ysh, at, len, lane, h0, hc, edges, scale, y32, y64);
    }
    if (nan_heads && lane == 0) atomicAdd(nan_pairs, (uint32_t)__popc(nan_heads));
    attn_wave_sync();
    sga_product<V_ET, V>(ysh, idsh, len, v, ldv, (uint64_t)h0 * dv, wc, dv, nan_heads, lane, o32, o64);
}

// The groups of the long path by column: their y of one head lies in position order (y[p], p a position of in_pos); this copies
// it to the y outputs in edge order, o[in_pos[p]] = y[p].  rows: one PropSeg per long group (first, len); o32 / o64 point at the
// head's first element, either may be null.  grid = (ceil(longest / BLOCK) capped, min(nrow, 65535)).
__global__ void __launch_bounds__(BLOCK) k_sub_attn_y_places(const PropSeg *rows, uint64_t nrow, const int64_t *__restrict__ pos, const double *y, float *o32,
                                                             double *o64) {
    for (uint64_t i = blockIdx.y; i < nrow; i += gridDim.y) {
        const PropSeg r = rows[i];
        for (uint32_t k = blockIdx.x * BLOCK + threadIdx.x; k < r.len; k += gridDim.x * BLOCK) {
            const double val = y[r.first + k];
            const int64_t e = pos[r.first + k];
            if (o64) o64[e] = val;
            if (o32) o32[e] = (float)val;
        }
    }
}

} // namespace fora
