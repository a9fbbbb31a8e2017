// fora_attn_bwd.h -- the fused kernels of ATTENTION, BACKWARD (fora_hip_sparse_attention_bwd; the contract is in
// include/fora_hip.h, the split of rows and columns in fora_attn_bwd_plan.h).  Per head the gradients are a composition of
// contracts that exist -- dy = SCORES (SDDMM) of (g, v); ds = ROW SOFTMAX backward of (y, dy); dq = PROPAGATE WITH VALUES of k
// with ds; dk and dv = PROPAGATE WITH VALUES, TRANSPOSED of q with ds and of g with y -- and the two kernels here are built
// from the device functions that define those bits, so that nothing leaves f64 and nothing is added in another order.
//   k_attn_bwd_short  the row side, the mirror of k_attn_short (fora_attn.h): one wave per (row of at most PROP_SEG entries,
//                     head).  dy by sddmm_scores over the g row and v, each to its entry's place in the wave's LDS; D and ds
//                     in registers by smax_bwd_load / smax_bwd_finish, lane l owning the places l, l + 64, l + 128, l + 192,
//                     y read from the caller's array; ds to the [heads][entries] buffer the column side reads, and back to
//                     LDS; dq by attn_product over k.  The row is one segment of every contract.
//   k_attn_cols       the column side: one lane group per (non-empty column of at most PROP_SEG entries, head), with
//                     prop_geom's groups -- G lanes hold a tile of G * V columns of the head's slice, a wave 64 / G units.
//                     acc = acc + values[head * entries + pos[p]] * feat[rows[p]][head * w + c] from +0.0 over the column's
//                     entries p in transposed order, PROP_INFLIGHT rows of feat in flight.  The column is one segment of
//                     PROPAGATE, TRANSPOSED, so out = P_0: no partial-sum buffer, no combine.  Launched once for dk (values
//                     = ds, feat = q) and once for dv (values = y, feat = g).  An empty column is in no list; the host has
//                     zeroed the outputs.
// A wave's LDS is its own -- 256 doubles and 256 ids -- and what one lane writes another reads only behind a wave-wide fence:
// no workgroup barrier, a wave with no work just leaves.
// Nothing is fused: the file is compiled with -ffp-contract=off and every kernel says so again itself.
#pragma once
#include "fora_attn.h" // attn_wave_sync, attn_product, ATTN_ROWS
#include "fora_attn_bwd_plan.h"

namespace fora {

// grid = ceil(nrow * heads / ATTN_ROWS) workgroups of BLOCK threads.  Wave u of the grid owns head u % heads of row u / heads
// of the list.  g: nq x heads * dv (the gradient of the output), v: n x heads * dv, k: n x heads * d -- the whole operands;
// lgv = log2 of the lane group that scores dv columns.  y: [heads][entries], f64 when y_f64, else f32 widened exactly.
// ds (null: no column side wants it): [heads][entries].  dq32 / dq64: nq x heads * d with their own pitches; both null: dq is
// not wanted and the product is skipped.  G_ET, V_ET: the types of g and v as sddmm_load takes them (types: sddmm_types() of the
// two, for ELT_ANY); K_ET: k's own type.
template <int G_ET, int V_ET, int K_ET, int V>
__global__ void __launch_bounds__(BLOCK) k_attn_bwd_short(const PropSeg *rows, uint64_t nrow, uint32_t heads, const int32_t *ids, const void *g, int64_t ldg,
                                                          const void *v, int64_t ldv, const void *k, int64_t ldk, uint32_t d, uint32_t dv, uint32_t lgv,
                                                          double scale, uint64_t entries, const void *y, bool y_f64, double *ds, float *dq32, int64_t ld32,
                                                          double *dq64, int64_t ld64, uint32_t types) {
#pragma clang fp contract(off)
    __shared__ double sh_s[ATTN_ROWS][PROP_SEG];
    __shared__ int32_t sh_id[ATTN_ROWS][PROP_SEG];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t u = (uint64_t)blockIdx.x * ATTN_ROWS + wave;
    if (u >= nrow * heads) return; // (the whole wave)
    const uint32_t head = (uint32_t)(u % heads);
    PropSeg sg = rows[u / heads];
    sg.len = min(sg.len, PROP_SEG); // (the host lists no longer row; a wave's LDS holds this many)
    double *const ssh = sh_s[wave];
    int32_t *const idsh = sh_id[wave];
    float *const o32 = dq32 ? dq32 + (int64_t)sg.row * ld32 + (uint64_t)head * d : nullptr;
    double *const o64 = dq64 ? dq64 + (int64_t)sg.row * ld64 + (uint64_t)head * d : nullptr;
    if (!sg.len) { // an empty row: +0.0
        for (uint32_t c = lane; c < d; c += 64u) {
            if (o64) o64[c] = 0.0;
            if (o32) o32[c] = 0.0f;
        }
        return;
    }
    // ---- dy, each to its entry's place
#pragma unroll
    for (uint32_t j = 0; j < SMAX_PER_LANE; j++)
        if (lane + 64u * j < sg.len) idsh[lane + 64u * j] = ids[sg.first + lane + 64u * j];
    sddmm_scores<G_ET, V_ET>(ids + sg.first, sg.len, g, (uint64_t)(uint32_t)sg.row * (uint64_t)ldg + (uint64_t)head * dv, v, ldv, (uint64_t)head * dv, dv, lgv, lane, types,
                                 [=](uint32_t e, double s) { ssh[e] = s; });
    attn_wave_sync();
    // ---- D and ds in registers: y from the caller's array, dy from LDS
    PropSeg rel = sg; // the row as a segment of the LDS array, and of the head's y and ds from the row's first entry on
    rel.first = 0;
    const uint64_t at = (uint64_t)head * entries + (uint64_t)sg.first;
    double yv[SMAX_PER_LANE], gv[SMAX_PER_LANE];
    const double D = y_f64 ? smax_bwd_load(rel, lane, (const double *)y + at, (const double *)ssh, yv, gv)
                           : smax_bwd_load(rel, lane, (const float *)y + at, (const double *)ssh, yv, gv);
    smax_bwd_finish(rel, lane, D, scale, yv, gv, nullptr, ds ? ds + at : nullptr); // (ds is left in yv)
    if (!o32 && !o64) return;
    attn_wave_sync(); // (every lane has read its dy before ds takes their place)
    smax_store(rel, lane, yv, nullptr, ssh);
    attn_wave_sync();
    // ---- dq
    attn_product<K_ET, V>(ssh, idsh, sg.len, k, ldk, (uint64_t)head * d, d, lane, o32, o64);
}

// grid = (ceil(ncol * heads / (units per workgroup)), column tiles), BLOCK threads; units per workgroup = (BLOCK / 64) * (64 / G).
// Unit u of the grid owns head u % heads of column u / heads of the list; lane gl of its group the columns
// [(blockIdx.y * G + gl) * V, ... + V) of the head's slice of w columns.  The body is prop_gather_body's (fora_prop.h) with
// the weights at values[head * entries + pos[p]] and the sum stored, not parked: a group reads G entries of its column at a
// time, one per lane, hands them round with a shuffle, and has the loads of PROP_INFLIGHT feat rows issued before the first is
// widened and added.  The adds follow the entry order.  out32 / out64: n x heads * w with their own pitches, either may be
// null.
template <int ET, int V, bool VAL64>
__global__ void __launch_bounds__(BLOCK) k_attn_cols(const PropSeg *cols, uint64_t ncol, uint32_t heads, const int32_t *rows, const int64_t *pos, const void *values,
                                                     uint64_t entries, const void *feat, int64_t ldf, uint32_t w, uint32_t G, float *out32, int64_t ld32,
                                                     double *out64, int64_t ld64) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t gl = lane & (G - 1u), grp = lane / G;
    const uint64_t u = ((uint64_t)blockIdx.x * (BLOCK / 64) + wave) * (64u / G) + grp;
    const uint32_t c0 = (blockIdx.y * G + gl) * (uint32_t)V;
    const uint32_t ncl = c0 < w ? min((uint32_t)V, w - c0) : 0u;
    const bool live = u < ncol * heads;
    uint32_t len = 0, head = 0;
    int32_t col = 0;
    int64_t first = 0;
    if (live) {
        const PropSeg sg = cols[u / heads];
        head = (uint32_t)(u % heads);
        len = min(sg.len, PROP_SEG); // (the host lists no longer column)
        first = sg.first;
        col = sg.row;
    }
    const uint64_t fcol = (uint64_t)head * w + c0, vat = (uint64_t)head * entries;
    double acc[V];
#pragma unroll
    for (int i = 0; i < V; i++) acc[i] = 0.0;
    for (uint32_t base = 0; base < len; base += G) {
        int32_t id_l = 0;
        double w_l = 0.0;
        if (base + gl < len) {
            id_l = rows[first + base + gl];
            const uint64_t e = vat + (uint64_t)pos[first + base + gl];
            if constexpr (VAL64) w_l = ((const double *)values)[e];
            else w_l = (double)((const float *)values)[e];
        }
        const uint32_t cnt = min(G, len - base);
        for (uint32_t k = 0; k < cnt; k += PROP_INFLIGHT) {
            PropRaw<ET, V> raw[PROP_INFLIGHT];
            uint64_t off[PROP_INFLIGHT];
            double wt[PROP_INFLIGHT];
#pragma unroll
            for (int t = 0; t < PROP_INFLIGHT; t++) {
                const int from = (int)min(k + (uint32_t)t, cnt - 1u);
                off[t] = (uint64_t)(uint32_t)__shfl(id_l, from, (int)G) * (uint64_t)ldf + fcol;
                wt[t] = __shfl(w_l, from, (int)G);
#pragma unroll
                for (int j = 0; j < PropRaw<ET, V>::W; j++) raw[t].w[j] = 0;
            }
            if (ncl == (uint32_t)V) { // (as in prop_gather_body: the choice stands outside the loop over the rows)
#pragma unroll
                for (int t = 0; t < PROP_INFLIGHT; t++)
                    if (k + (uint32_t)t < cnt) prop_load_full<ET, V>(feat, off[t], raw[t]);
            } else if (ncl) {
#pragma unroll
                for (int t = 0; t < PROP_INFLIGHT; t++)
                    if (k + (uint32_t)t < cnt) prop_load_tail<ET, V>(feat, off[t], ncl, raw[t]);
            }
#pragma unroll
            for (int t = 0; t < PROP_INFLIGHT; t++) {
                const bool valid = k + (uint32_t)t < cnt;
#pragma unroll
                for (int i = 0; i < V; i++) {
                    const double term = wt[t] * prop_widen<ET, V>(raw[t], i);
                    const double sum = acc[i] + term;
                    acc[i] = valid ? sum : acc[i];
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int i = 0; i < V; i++) {
            if ((uint32_t)i < ncl) {
                if (out64) out64[(int64_t)col * ld64 + (int64_t)(fcol + (uint32_t)i)] = acc[i];
                if (out32) out32[(int64_t)col * ld32 + (int64_t)(fcol + (uint32_t)i)] = (float)acc[i];
            }
        }
    }
}

} // namespace fora
