// fora_subgraph_pool.h -- the kernels of SUBGRAPH POOL (fora_hip_subgraph_pool, fora_hip_subgraph_pool_bwd; the contract is in
// include/fora_hip_pool.h): the element-wise maximum or minimum over a node's neighbours in the held subgraph with the edge
// that gave it, and the gradient that goes to that edge alone -- every bit defined, ties included.
//   k_sub_pool          the groups of at most `cap` entries, the empty ones included: one lane group per (group, column tile) on
//                       the lane map of k_sub_agg (prop_geom), its loads (PROP_INFLIGHT rows in flight), and in place of a sum V
//                       running (key, place) pairs a lane -- the group's winners under the contract's total order;
//   k_sub_pool_long     a longer group (a hub): one workgroup per (group, column tile), its lane groups striding over the entries,
//                       the pairs merged across a wave's lane groups by shuffles and across the waves through LDS -- one launch,
//                       no partial result in device memory;
//   k_sub_pool_bwd      the across groups of at most `cap` entries: per entry the tiles of g[j] and of arg[j], the term
//                       (arg == e) ? g : +0.0 -- a select -- added in entry order from +0.0 in f64 registers, the stores;
//   k_sub_pool_bwd_seg  the same sum over the segments of the side's long plan into the chunk's partial sums; k_prop_combine
//                       (fora_prop.h) follows as it does behind every gather.
// A winner is tracked by its PLACE INSIDE ITS GROUP (a group holds fewer than 2^32 entries), not by its edge: places ascend as
// the edges do under both groupings, they need no shuffle, and by column in_pos is read once per output element at the store,
// not once per entry.  The maximum and the minimum are one code path: the key of an entry is its value with the sign bit
// flipped for the minimum -- exact and undone at the store -- so that "first under IEEE >" is the order of both.
// Nothing here is fused: the file is compiled with -ffp-contract=off and the backward kernels say so again themselves.
#pragma once
#include "fora_subgraph_prop.h"

namespace fora {

constexpr uint32_t POOL_NONE = 0xFFFFFFFFu;             // the place of a pair that has met no entry yet
constexpr uint64_t POOL_QNAN = 0x7FF8000000000000ull;   // what a NaN winner is written as
constexpr uint64_t POOL_SIGN = 0x8000000000000000ull;

__device__ __forceinline__ double pool_flip(double t, uint64_t flip) { return __longlong_as_double((long long)((uint64_t)__double_as_longlong(t) ^ flip)); }

// the contract's total order on keys: does (kb, ib) stand before (ka, ia)?  A NaN before every number, the larger key before
// the smaller, -0.0 and +0.0 equal, every tie (among NaNs too) to the smaller place; a pair without an entry stands behind all
__device__ __forceinline__ bool pool_before(double kb, uint32_t ib, double ka, uint32_t ia) {
    const bool an = ka != ka, bn = kb != kb;
    const bool b_first = (bn & !an) | (kb > ka), a_first = (an & !bn) | (ka > kb);
    return ib != POOL_NONE && (ia == POOL_NONE || b_first || (!a_first && ib < ia));
}

// The entries start, start + 1 .. start + G - 1, then stride further on, of the group [first, first + len): ids read one per lane
// and handed round the lane group, up to PROP_INFLIGHT feature rows loaded before the first is widened, as k_sub_agg does.  The
// places a lane group meets ascend, so a later entry takes a pair over only where it stands strictly before its holder.
template <int ET, int V>
__device__ __forceinline__ void pool_scan(const int32_t *ids, const void *feat, int64_t ldf, int64_t first, uint32_t start, uint32_t len, uint32_t stride,
                                          uint32_t G, uint32_t gl, uint32_t c0, uint32_t ncol, uint64_t flip, double (&bk)[V], uint32_t (&bi)[V]) {
    for (uint64_t base = start; base < len; base += stride) {
        int32_t id_l = 0;
        if (base + gl < len) id_l = ids[first + (int64_t)base + gl];
        const uint32_t cnt = min(G, len - (uint32_t)base);
        for (uint32_t k = 0; k < cnt; k += PROP_INFLIGHT) {
            PropRaw<ET, V> raw[PROP_INFLIGHT];
            uint64_t off[PROP_INFLIGHT];
#pragma unroll
            for (int u = 0; u < PROP_INFLIGHT; u++) {
                const int from = (int)min(k + (uint32_t)u, cnt - 1u);
                off[u] = (uint64_t)(uint32_t)__shfl(id_l, from, (int)G) * (uint64_t)ldf + c0;
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
                const uint32_t place = (uint32_t)base + k + (uint32_t)u;
#pragma unroll
                for (int v = 0; v < V; v++) {
                    const double key = pool_flip(prop_widen<ET, V>(raw[u], v), flip);
                    const bool take = valid & ((bi[v] == POOL_NONE) | ((key != key) & (bk[v] == bk[v])) | (key > bk[v]));
                    bk[v] = take ? key : bk[v];
                    bi[v] = take ? place : bi[v];
                }
            }
        }
    }
}

// the winners of group r written: the value bit for bit (a NaN as POOL_QNAN), rounded once for out32, and the edge -- first + place
// by row, in_pos[first + place] by column (pos); a group without entries is +0.0 and -1
template <int V>
__device__ __forceinline__ void pool_store(uint64_t r, int64_t first, const int64_t *pos, uint32_t c0, uint32_t ncol, uint64_t flip, const double (&bk)[V],
                                           const uint32_t (&bi)[V], float *out32, int64_t ld32, double *out64, int64_t ld64, int32_t *arg, int64_t lda) {
#pragma unroll
    for (int v = 0; v < V; v++) {
        if ((uint32_t)v >= ncol) continue;
        const bool none = bi[v] == POOL_NONE;
        const double a = none ? 0.0 : (bk[v] != bk[v] ? __longlong_as_double((long long)POOL_QNAN) : pool_flip(bk[v], flip));
        if (out64) out64[(int64_t)r * ld64 + c0 + (uint32_t)v] = a;
        if (out32) out32[(int64_t)r * ld32 + c0 + (uint32_t)v] = (float)a;
        if (arg) {
            int64_t e = -1;
            if (!none) { e = first + (int64_t)bi[v]; if (pos) e = pos[e]; }
            arg[(int64_t)r * lda + c0 + (uint32_t)v] = (int32_t)e;
        }
    }
}

// grid = (ceil(rows / (rows per workgroup)), column tiles), BLOCK threads, the lane map of k_sub_agg.  ptr: sub_ptr by row, in_ptr
// by column; ids: sub_col / in_row, the feature row of every entry; pos: null by row, in_pos by column.  neg: 1 the minimum
// (uniform over the grid).  A group longer than cap is not touched.  No bit depends on G, V or the grid.
template <int ET, int V>
__global__ void __launch_bounds__(BLOCK) k_sub_pool(const int64_t *ptr, uint32_t rows, uint32_t cap, const int32_t *ids, const int64_t *pos, const void *feat, int64_t ldf,
                                                    uint32_t d, uint32_t G, uint32_t neg, float *out32, int64_t ld32, double *out64, int64_t ld64, int32_t *arg,
                                                    int64_t lda) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t gl = lane & (G - 1u), grp = lane / G;
    const uint64_t r = ((uint64_t)blockIdx.x * (BLOCK / 64) + wave) * (64u / G) + grp;
    const uint32_t c0 = (blockIdx.y * G + gl) * (uint32_t)V;
    const uint32_t ncol = c0 < d ? min((uint32_t)V, d - c0) : 0u;
    const uint64_t flip = neg ? POOL_SIGN : 0ull;
    uint32_t len = 0;
    int64_t first = 0;
    bool mine = false;
    if (r < rows) {
        first = ptr[r];
        const uint64_t n = (uint64_t)(ptr[r + 1] - first);
        mine = n <= (uint64_t)cap;
        len = mine ? (uint32_t)n : 0u;
    }
    double bk[V];
    uint32_t bi[V];
#pragma unroll
    for (int v = 0; v < V; v++) { bk[v] = 0.0; bi[v] = POOL_NONE; }
    pool_scan<ET, V>(ids, feat, ldf, first, 0u, len, G, G, gl, c0, ncol, flip, bk, bi);
    if (mine) pool_store<V>(r, first, pos, c0, ncol, flip, bk, bi, out32, ld32, out64, ld64, arg, lda);
}

// grid = (long groups, column tiles), BLOCK threads, (BLOCK / 64 - 1) * G * V * 12 bytes of dynamic LDS.  list: the side's groups
// longer than the cap.  Thread t is lane t % G of lane group t / G -- BLOCK / G lane groups, which between them read BLOCK
// adjacent ids at a time, so lane group q scans the entries q * G .. q * G + G - 1, then BLOCK further on.  The pairs of a
// wave's lane groups meet by xor shuffles at strides G .. 32 (every lane ends with the wave's winners), those of the waves 1 ..
// in LDS as [wave - 1][v][lane] -- adjacent lanes adjacent words -- behind the one barrier; lane group 0 merges and stores.
// The order is total, so the pairing of the merges changes no bit.
template <int ET, int V>
__global__ void __launch_bounds__(BLOCK) k_sub_pool_long(const int64_t *ptr, const int32_t *list, const int32_t *ids, const int64_t *pos, const void *feat, int64_t ldf,
                                                         uint32_t d, uint32_t G, uint32_t neg, float *out32, int64_t ld32, double *out64, int64_t ld64, int32_t *arg,
                                                         int64_t lda) {
    extern __shared__ double pool_lds[];
    constexpr uint32_t WAVES = BLOCK / 64;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t gl = threadIdx.x & (G - 1u), lg = threadIdx.x / G;
    const uint64_t r = (uint64_t)(uint32_t)list[blockIdx.x];
    const uint32_t c0 = (blockIdx.y * G + gl) * (uint32_t)V;
    const uint32_t ncol = c0 < d ? min((uint32_t)V, d - c0) : 0u;
    const uint64_t flip = neg ? POOL_SIGN : 0ull;
    const int64_t first = ptr[r];
    const uint32_t len = (uint32_t)(ptr[r + 1] - first);
    double bk[V];
    uint32_t bi[V];
#pragma unroll
    for (int v = 0; v < V; v++) { bk[v] = 0.0; bi[v] = POOL_NONE; }
    pool_scan<ET, V>(ids, feat, ldf, first, lg * G, len, (uint32_t)BLOCK, G, gl, c0, ncol, flip, bk, bi);
    for (uint32_t o = G; o < 64u; o <<= 1) {
#pragma unroll
        for (int v = 0; v < V; v++) {
            const double ok = __shfl_xor(bk[v], (int)o);
            const uint32_t oi = (uint32_t)__shfl_xor((int)bi[v], (int)o);
            const bool take = pool_before(ok, oi, bk[v], bi[v]);
            bk[v] = take ? ok : bk[v];
            bi[v] = take ? oi : bi[v];
        }
    }
    uint32_t *lds_i = (uint32_t *)(pool_lds + (size_t)(WAVES - 1u) * V * G);
    if (wave && lane < G) {
#pragma unroll
        for (int v = 0; v < V; v++) {
            pool_lds[((wave - 1u) * V + (uint32_t)v) * G + lane] = bk[v];
            lds_i[((wave - 1u) * V + (uint32_t)v) * G + lane] = bi[v];
        }
    }
    __syncthreads();
    if (wave || lane >= G) return;
    for (uint32_t w = 0; w + 1u < WAVES; w++) {
#pragma unroll
        for (int v = 0; v < V; v++) {
            const double ok = pool_lds[(w * V + (uint32_t)v) * G + lane];
            const uint32_t oi = lds_i[(w * V + (uint32_t)v) * G + lane];
            const bool take = pool_before(ok, oi, bk[v], bi[v]);
            bk[v] = take ? ok : bk[v];
            bi[v] = take ? oi : bi[v];
        }
    }
    pool_store<V>(r, first, pos, c0, ncol, flip, bk, bi, out32, ld32, out64, ld64, arg, lda);
}

// V adjacent int32 of one row of arg.  wide (the host saw base and pitch aligned to min(V, 4) words): a full tile in loads of 16
// bytes (8 with V == 2); else, and in a tile's last lane, one by one -- a column that does not exist names no edge (-1)
template <int V>
__device__ __forceinline__ void pool_load_arg(const int32_t *arg, uint64_t off, uint32_t ncol, bool wide, int32_t (&a)[V]) {
    if (wide && ncol == (uint32_t)V) {
        if constexpr (V >= 4) {
#pragma unroll
            for (int q = 0; q < V / 4; q++) { const int4 x = *(const int4 *)(arg + off + 4 * q); a[4 * q] = x.x; a[4 * q + 1] = x.y; a[4 * q + 2] = x.z; a[4 * q + 3] = x.w; }
        } else if constexpr (V == 2) { const int2 x = *(const int2 *)(arg + off); a[0] = x.x; a[1] = x.y; }
        else a[0] = arg[off];
    } else {
#pragma unroll
        for (int v = 0; v < V; v++) a[v] = (uint32_t)v < ncol ? arg[off + (uint32_t)v] : -1;
    }
}

// acc[v] += (arg[j][c0 + v] == e) ? widen(g[j][c0 + v]) : +0.0 over the entries [first, first + len) in order, j = ids[entry] and
// e = pos[entry], or the entry's own place in sub_col where pos is null.  arg is compared as the 64-bit e it would name.
template <int ET, int V>
__device__ __forceinline__ void pool_bwd_sum(const int32_t *ids, const int64_t *pos, int64_t first, uint32_t len, const void *g, int64_t ldg, const int32_t *arg,
                                             int64_t lda, bool wide, uint32_t G, uint32_t gl, uint32_t c0, uint32_t ncol, double (&acc)[V]) {
#pragma clang fp contract(off)
    for (uint32_t base = 0; base < len; base += G) {
        int32_t id_l = 0;
        long long e_l = 0;
        if (base + gl < len) {
            const int64_t at = first + base + gl;
            id_l = ids[at];
            e_l = pos ? pos[at] : at;
        }
        const uint32_t cnt = min(G, len - base);
        for (uint32_t k = 0; k < cnt; k += PROP_INFLIGHT) {
            PropRaw<ET, V> raw[PROP_INFLIGHT];
            int32_t a[PROP_INFLIGHT][V];
            uint64_t row[PROP_INFLIGHT];
            long long e[PROP_INFLIGHT];
#pragma unroll
            for (int u = 0; u < PROP_INFLIGHT; u++) {
                const int from = (int)min(k + (uint32_t)u, cnt - 1u);
                row[u] = (uint64_t)(uint32_t)__shfl(id_l, from, (int)G);
                e[u] = __shfl(e_l, from, (int)G);
#pragma unroll
                for (int j = 0; j < PropRaw<ET, V>::W; j++) raw[u].w[j] = 0;
#pragma unroll
                for (int v = 0; v < V; v++) a[u][v] = -1;
            }
            if (ncol == (uint32_t)V) {
#pragma unroll
                for (int u = 0; u < PROP_INFLIGHT; u++)
                    if (k + (uint32_t)u < cnt) prop_load_full<ET, V>(g, row[u] * (uint64_t)ldg + c0, raw[u]);
            } else if (ncol) {
#pragma unroll
                for (int u = 0; u < PROP_INFLIGHT; u++)
                    if (k + (uint32_t)u < cnt) prop_load_tail<ET, V>(g, row[u] * (uint64_t)ldg + c0, ncol, raw[u]);
            }
            if (ncol) {
#pragma unroll
                for (int u = 0; u < PROP_INFLIGHT; u++)
                    if (k + (uint32_t)u < cnt) pool_load_arg<V>(arg, row[u] * (uint64_t)lda + c0, ncol, wide, a[u]);
            }
#pragma unroll
            for (int u = 0; u < PROP_INFLIGHT; u++) {
                const bool valid = k + (uint32_t)u < cnt;
#pragma unroll
                for (int v = 0; v < V; v++) {
                    const double term = (long long)a[u][v] == e[u] ? prop_widen<ET, V>(raw[u], v) : 0.0;
                    const double sum = acc[v] + term;
                    acc[v] = valid ? sum : acc[v];
                }
            }
        }
    }
}

// grid and lane map of k_sub_pool over the ACROSS groups: ptr in_ptr, ids in_row and pos in_pos for a forward call by row; ptr
// sub_ptr, ids sub_col and pos null for one by column.  A group longer than cap (at most PROP_SEG: one segment) is not touched.
template <int ET, int V>
__global__ void __launch_bounds__(BLOCK) k_sub_pool_bwd(const int64_t *ptr, uint32_t rows, uint32_t cap, const int32_t *ids, const int64_t *pos, const void *g, int64_t ldg,
                                                        uint32_t d, uint32_t G, const int32_t *arg, int64_t lda, uint32_t wide, float *out32, int64_t ld32, double *out64,
                                                        int64_t ld64) {
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
    pool_bwd_sum<ET, V>(ids, pos, first, len, g, ldg, arg, lda, wide != 0u, G, gl, c0, ncol, acc);
    if (!mine) return;
#pragma unroll
    for (int v = 0; v < V; v++) {
        if ((uint32_t)v >= ncol) continue;
        if (out64) out64[(int64_t)r * ld64 + c0 + (uint32_t)v] = acc[v];
        if (out32) out32[(int64_t)r * ld32 + c0 + (uint32_t)v] = (float)acc[v];
    }
}

// the long path: grid and lane map of k_prop_gather over the segments of the side's long plan, the sum of segment s to
// part[slot][d] -- what k_prop_combine adds up in segment order
template <int ET, int V>
__global__ void __launch_bounds__(BLOCK) k_sub_pool_bwd_seg(const PropSeg *segs, uint64_t nseg, const int32_t *ids, const int64_t *pos, const void *g, int64_t ldg, uint32_t d,
                                                            uint32_t G, const int32_t *arg, int64_t lda, uint32_t wide, double *part) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t gl = lane & (G - 1u), grp = lane / G;
    const uint64_t s = ((uint64_t)blockIdx.x * (BLOCK / 64) + wave) * (64u / G) + grp;
    const uint32_t c0 = (blockIdx.y * G + gl) * (uint32_t)V;
    const uint32_t ncol = c0 < d ? min((uint32_t)V, d - c0) : 0u;
    uint32_t len = 0, slot = 0;
    int64_t first = 0;
    if (s < nseg) { const PropSeg sg = segs[s]; len = sg.len; slot = sg.slot; first = sg.first; }
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; v++) acc[v] = 0.0;
    pool_bwd_sum<ET, V>(ids, pos, first, len, g, ldg, arg, lda, wide != 0u, G, gl, c0, ncol, acc);
    if (s >= nseg) return;
#pragma unroll
    for (int v = 0; v < V; v++)
        if ((uint32_t)v < ncol) part[(uint64_t)slot * d + c0 + (uint32_t)v] = acc[v];
}

} // namespace fora
