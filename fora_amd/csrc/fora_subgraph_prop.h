// fora_subgraph_prop.h -- the kernels of SUBGRAPH PRODUCTS (fora_hip_subgraph_propagate, fora_hip_subgraph_propagate_t; the
// contract is in include/fora_hip_gnn.h, the split in fora_subgraph_prop_plan.h): out = A_S x X over the rows of the held
// subgraph, out = A_S^T x G over its transposition, every bit defined.
//   k_subt_count      cnt[sub_col[e]] += 1 per edge (u32 atomics: the sum does not depend on their order);
//   (the host turns cnt into in_ptr; k_propt_place and the three sort tiers of fora_propt.h put every column's keys in order)
//   k_subt_fill       in_row[p] = key >> 32, in_pos[p] = sub_ptr[row] + the key's low word: the edge's place in sub_col;
//   k_sub_agg         the fused product of the output rows of at most `cap` entries: one lane group per (row, column tile),
//                     the terms added in entry order from +0.0 in f64 registers, the MEAN division, the stores -- no partial
//                     sums, no second launch, no table from the host; a longer row is left to the long path;
//   k_sub_gather_one  the gather of PROPAGATE (prop_gather_body) with every weight 1.0, for the long path without values.
// Nothing here is fused: the file is compiled with -ffp-contract=off and the kernels say so again themselves.
#pragma once
#include "fora_prop.h"
#include "fora_propt.h"
#include "fora_subgraph_prop_plan.h"

namespace fora {

// a workgroup per row (grid-stride): the row's targets counted
__global__ void __launch_bounds__(BLOCK) k_subt_count(const int64_t *sub_ptr, uint32_t nc, const int32_t *sub_col, uint32_t *cnt) {
    for (uint32_t i = blockIdx.x; i < nc; i += gridDim.x) {
        const int64_t lo = sub_ptr[i], hi = sub_ptr[i + 1];
        for (int64_t e = lo + threadIdx.x; e < hi; e += BLOCK) {
            const uint32_t v = (uint32_t)sub_col[e];
            if (v < nc) atomicAdd(&cnt[v], 1u);
        }
    }
}

__global__ void __launch_bounds__(BLOCK) k_subt_fill(const uint64_t *key, uint64_t edges, const int64_t *sub_ptr, uint32_t nc, int32_t *in_row, int64_t *in_pos) {
    for (uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; p < edges; p += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t kk = key[p];
        const uint32_t i = (uint32_t)(kk >> 32);
        if (i >= nc) continue; // (a key nobody wrote: cannot happen with counts and places of one subgraph)
        const uint64_t at = (uint64_t)sub_ptr[i] + (kk & 0xFFFFFFFFull);
        if (at >= edges) continue;
        in_row[p] = (int32_t)i;
        in_pos[p] = (int64_t)at;
    }
}

// grid = (ceil(rows / (rows per workgroup)), column tiles), BLOCK threads, the lane map of k_prop_gather (prop_geom): group g of
// wave w of workgroup x owns output row (x * BLOCK / 64 + w) * (64 / G) + g and the columns [(y * G + gl) * V, ... + V) on lane gl.
// ptr: sub_ptr forward, in_ptr transposed (device memory, read here); ids: sub_col / in_row, the feature row of every entry;
// pos: null forward, in_pos transposed -- where an entry's value lies; wmode 0: every weight 1.0, 1: f32 values, 2: f64 values.
// A row longer than cap (at most PROP_SEG: one segment) is not touched.  mean: the finished sum divided once by the row's
// number of terms; a row without terms is +0.0.  The adds follow the entry order, so no bit depends on G, V or the grid.
template <int ET, int V>
__global__ void __launch_bounds__(BLOCK) k_sub_agg(const int64_t *ptr, uint32_t rows, uint32_t cap, const int32_t *ids, const int64_t *pos, const void *values,
                                                   uint32_t wmode, const void *feat, int64_t ldf, uint32_t d, uint32_t G, uint32_t mean, float *out32, int64_t ld32,
                                                   double *out64, int64_t ld64) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t gl = lane & (G - 1u), grp = lane / G;
    const uint64_t r = ((uint64_t)blockIdx.x * (BLOCK / 64) + wave) * (64u / G) + grp;
    const uint32_t c0 = (blockIdx.y * G + gl) * (uint32_t)V;
    const uint32_t ncol = c0 < d ? min((uint32_t)V, d - c0) : 0u;
    uint32_t len = 0;
    int64_t first = 0;
    bool mine = false;
    if (r < rows) {
        first = ptr[r];
        const uint64_t n = (uint64_t)(ptr[r + 1] - first);
        mine = n <= (uint64_t)cap;
        len = mine ? (uint32_t)n : 0u;
    }
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; v++) acc[v] = 0.0;
    for (uint32_t base = 0; base < len; base += G) {
        int32_t id_l = 0;
        double w_l = 1.0;
        if (base + gl < len) {
            int64_t at = first + base + gl;
            id_l = ids[at];
            if (wmode) {
                if (pos) at = pos[at];
                w_l = wmode == 2u ? ((const double *)values)[at] : (double)((const float *)values)[at];
            }
        }
        const uint32_t cnt = min(G, len - base);
        for (uint32_t k = 0; k < cnt; k += PROP_INFLIGHT) {
            PropRaw<ET, V> raw[PROP_INFLIGHT];
            uint64_t off[PROP_INFLIGHT];
            double w[PROP_INFLIGHT];
#pragma unroll
            for (int u = 0; u < PROP_INFLIGHT; u++) {
                const int from = (int)min(k + (uint32_t)u, cnt - 1u);
                off[u] = (uint64_t)(uint32_t)__shfl(id_l, from, (int)G) * (uint64_t)ldf + c0;
                w[u] = __shfl(w_l, from, (int)G);
#pragma unroll
                for (int j = 0; j < PropRaw<ET, V>::W; j++) raw[u].w[j] = 0;
            }
            if (ncol == (uint32_t)V) {
#pragma unroll
                for (int u = 0; u < PROP_INFLIGHT; u++)
                    if (k + (uint32_t)u < cnt) prop_load_full<ET, V>(feat, off[u], raw[u]);
            } else if (ncol) {
#pragma unroll
                for (int u = 0; u < PROP_INFLIGHT; u++)
                    if (k + (uint32_t)u < cnt) prop_load_tail<ET, V>(feat, off[u], ncol, raw[u]);
            }
#pragma unroll
            for (int u = 0; u < PROP_INFLIGHT; u++) {
                const bool valid = k + (uint32_t)u < cnt;
#pragma unroll
                for (int v = 0; v < V; v++) {
                    const double term = w[u] * prop_widen<ET, V>(raw[u], v);
                    const double sum = acc[v] + term;
                    acc[v] = valid ? sum : acc[v];
                }
            }
        }
    }
    if (!mine) return;
    const double terms = (double)len;
#pragma unroll
    for (int v = 0; v < V; v++) {
        if ((uint32_t)v >= ncol) continue;
        double a = acc[v];
        if (mean && len) a = a / terms;
        if (out64) out64[(int64_t)r * ld64 + c0 + (uint32_t)v] = a;
        if (out32) out32[(int64_t)r * ld32 + c0 + (uint32_t)v] = (float)a;
    }
}

// the long path without values: PROPAGATE's gather, every weight exactly 1.0 (no array of ones)
template <int ET, int V>
__global__ void __launch_bounds__(BLOCK) k_sub_gather_one(const PropSeg *segs, uint64_t nseg, const int32_t *ids, const void *feat, int64_t ldf, uint32_t d, uint32_t G,
                                                          double *part) {
    prop_gather_body<ET, V, false, PROP_W_ONE>(segs, nseg, ids, nullptr, feat, ldf, d, G, part, nullptr, nullptr);
}

} // namespace fora
