// fora_sweep.h -- local clustering: the sweep cut over a PPR row (Andersen-Chung-Lang), gfx950.  The SWEEP CUT contract of
// include/fora_hip.h; the host side is the batch plan of fora_sweep_plan.h and sweep_* in fora_hip.hip.
//
//   compaction   k_sparse_count / k_sparse_write (fora_kernels.h) into the sweep's own buffers, then k_sweep_keys
//   sort         k_sweep_sort_lds (a tile of a row in LDS: every bitonic step whose stride fits the tile),
//                k_sweep_sort_step (one step of a larger stride, in global memory)
//   rank map     k_sweep_scatter<true> / <false> (rank[slot][n], -1 between uses: set and reset over the same L ids)
//   cut count    k_sweep_cut (one gather of rank per out-edge of a profile node; +1 / -1 into a difference array)
//   profile      k_sweep_scan (both inclusive scans and the exact argmin of cut / den, one workgroup per row)
//
// Everything is an integer: the key floor(ppr / max(outdeg, 1)) sorts descending with ties by ascending id, a strict order
// (ids inside a row are distinct), so any correct sort gives the same bits; the cut counts are integer adds, so the order of
// the atomics changes nothing.
#pragma once
#include "fora_kernels.h"
#include "fora_sweep_plan.h" // SW_TILE_MAX and the records SweepRowDesc, SweepTile, SweepGRow, SweepRowOut

namespace fora {

constexpr int32_t SW_PAD_ID = 0x7FFFFFFF; // sentinel (key 0, this id): after every real entry, n <= 2^31 - 1
constexpr int SW_SCAN_ITEMS = 4;          // k_sweep_scan: consecutive positions per lane and step

// key descending, ties id ascending
__device__ __forceinline__ bool sw_before(uint64_t ka, int32_t ia, uint64_t kb, int32_t ib) { return ka > kb || (ka == kb && ia < ib); }

// fix -> key over the padded copies (the ids and words k_sparse_write left), sentinels behind them; grid = (X, rows)
__global__ void __launch_bounds__(BLOCK) k_sweep_keys(const SweepRowDesc *rows, const uint32_t *deg, uint32_t n, int32_t *ids, uint64_t *key, uint64_t cap) {
    const SweepRowDesc rd = rows[blockIdx.y];
    for (uint32_t j = blockIdx.x * BLOCK + threadIdx.x; j < rd.P; j += gridDim.x * BLOCK) {
        const uint64_t at = (uint64_t)rd.tbase + j;
        if (at >= cap) return;
        if (j < rd.len) {
            const uint32_t v = (uint32_t)ids[at];
            const uint32_t d = v < n ? deg[v] : 1u;
            key[at] = key[at] / (uint64_t)(d ? d : 1u);
        } else {
            ids[at] = SW_PAD_ID; key[at] = 0;
        }
    }
}

// Bitonic steps inside one tile of S = min(P, T) entries.  kk == 0: the whole network up to k = S (a row of P <= T is sorted
// by it); kk >= 2 T: the steps j = S / 2 .. 1 of stage kk.  A run of 2 k entries is "up" (sweep order) where bit k of the
// entry's index in its row is clear.
__global__ void __launch_bounds__(BLOCK) k_sweep_sort_lds(int32_t *ids, uint64_t *key, uint64_t cap, const SweepTile *tiles, uint32_t T, uint32_t kk) {
    __shared__ uint64_t s_key[SW_TILE_MAX];
    __shared__ int32_t s_id[SW_TILE_MAX];
    const SweepTile t = tiles[blockIdx.x];
    const uint32_t S = min(min(t.P, T), SW_TILE_MAX);
    if (kk > t.P || (uint64_t)t.base + S > cap) return; // (the same in every lane)
    for (uint32_t i = threadIdx.x; i < S; i += BLOCK) { s_key[i] = key[t.base + i]; s_id[i] = ids[t.base + i]; }
    __syncthreads();
    for (uint32_t k = kk ? kk : 2; k <= (kk ? kk : S); k <<= 1) {
        for (uint32_t j = min(k, S) >> 1; j; j >>= 1) {
            for (uint32_t p = threadIdx.x; p < (S >> 1); p += BLOCK) {
                const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const bool up = ((t.off + i) & k) == 0;
                const uint64_t ka = s_key[i], kb = s_key[l];
                const int32_t ia = s_id[i], ib = s_id[l];
                if (up ? sw_before(kb, ib, ka, ia) : sw_before(ka, ia, kb, ib)) {
                    s_key[i] = kb; s_id[i] = ib; s_key[l] = ka; s_id[l] = ia;
                }
            }
            __syncthreads();
        }
        if (k == 0x80000000u) break;
    }
    for (uint32_t i = threadIdx.x; i < S; i += BLOCK) { key[t.base + i] = s_key[i]; ids[t.base + i] = s_id[i]; }
}

// step (k, j) of the rows of the global tier, j at least a tile; grid = (X, rows); a row of P < k has no such step
__global__ void __launch_bounds__(BLOCK) k_sweep_sort_step(int32_t *ids, uint64_t *key, uint64_t cap, const SweepGRow *rows, uint32_t k, uint32_t j) {
    const SweepGRow r = rows[blockIdx.y];
    if (k > r.P || (uint64_t)r.base + r.P > cap) return;
    for (uint32_t p = blockIdx.x * BLOCK + threadIdx.x; p < (r.P >> 1); p += gridDim.x * BLOCK) {
        const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
        const bool up = (i & k) == 0;
        const uint64_t ka = key[r.base + i], kb = key[r.base + l];
        const int32_t ia = ids[r.base + i], ib = ids[r.base + l];
        if (up ? sw_before(kb, ib, ka, ia) : sw_before(ka, ia, kb, ib)) {
            key[r.base + i] = kb; ids[r.base + i] = ib; key[r.base + l] = ka; ids[r.base + l] = ia;
        }
    }
}

// The first L nodes of every row of a chunk (rows r0 + y, y = blockIdx.y, rank slab y).  SET: rank[node] = position, and the
// row's profile starts its life in the held arrays: order = the node, cut = 0 (the difference array k_sweep_cut adds into),
// vol = outdeg(node).  !SET: rank[node] = -1 again.  grid = (X, rows of the chunk)
template <bool SET>
__global__ void __launch_bounds__(BLOCK) k_sweep_scatter(const SweepRowDesc *rows, uint32_t r0, int32_t *rank_all, uint32_t n, const int32_t *t_ids, uint64_t tcap,
                                                         const uint32_t *deg, int32_t *h_ids, uint64_t *h_cut, uint64_t *h_vol, uint64_t hcap) {
    const SweepRowDesc rd = rows[r0 + blockIdx.y];
    int32_t *rank = rank_all + (uint64_t)blockIdx.y * n;
    for (uint32_t j = blockIdx.x * BLOCK + threadIdx.x; j < rd.L; j += gridDim.x * BLOCK) {
        const uint64_t ta = (uint64_t)rd.tbase + j, ha = (uint64_t)rd.hbase + j;
        if (ta >= tcap) return;
        const uint32_t v = (uint32_t)t_ids[ta];
        if (v >= n) continue; // (a sentinel: never among the first L <= len entries of a sorted row)
        if (SET) {
            rank[v] = (int32_t)j;
            if (ha < hcap) { h_ids[ha] = (int32_t)v; h_cut[ha] = 0; h_vol[ha] = deg[v]; }
        } else
            rank[v] = -1;
    }
}

// Out-edges u -> v of the node u at position i: r = rank[v]; v outside the profile or behind u (r < 0 or r > i) makes the
// edge a cut edge of every prefix from i on -- + 1 at i -- until v joins at r -- - 1 at r.  The + 1s of a node are summed
// first (in registers, over a wave, over the workgroup) and added once.  A workgroup takes BLOCK positions at a time: a lane
// walks the edges of its own node when there are fewer than 64, a wave those of a node with 64 .. BLOCK - 1, the whole
// workgroup those of a node with more.  diff is the row's cut array (i64 in two's complement, scanned by k_sweep_scan).
// grid = (X, rows of the chunk)
__global__ void __launch_bounds__(BLOCK) k_sweep_cut(const SweepRowDesc *rows, uint32_t r0, const int32_t *rank_all, uint32_t n, const int64_t *row_ptr,
                                                     const int32_t *col, const int32_t *h_ids, unsigned long long *diff, uint64_t hcap) {
    __shared__ uint32_t s_med[BLOCK], s_big[BLOCK];
    __shared__ uint32_t s_nmed, s_nbig, s_cnt;
    const SweepRowDesc rd = rows[r0 + blockIdx.y];
    const int32_t *rank = rank_all + (uint64_t)blockIdx.y * n;
    const uint32_t L = rd.L;
    if ((uint64_t)rd.hbase + L > hcap) return;
    const int32_t *order = h_ids + rd.hbase;
    unsigned long long *d = diff + rd.hbase;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const auto edge = [&](int64_t e, uint32_t pos, uint32_t &cnt) {
        const int32_t r = rank[(uint32_t)col[e]];
        if (r < 0 || r > (int32_t)pos) {
            cnt++;
            if (r > (int32_t)pos) atomicAdd(&d[r], ~0ull); // (r < L: only positions below L are in the map)
        }
    };
    for (uint32_t t0 = blockIdx.x * BLOCK; t0 < L; t0 += gridDim.x * BLOCK) { // (t0: the same in every lane)
        if (threadIdx.x == 0) { s_nmed = 0; s_nbig = 0; }
        __syncthreads();
        const uint32_t pos = t0 + threadIdx.x;
        if (pos < L) {
            const uint32_t u = (uint32_t)order[pos];
            const int64_t beg = row_ptr[u], dg = row_ptr[u + 1] - beg;
            if (dg >= BLOCK) s_big[atomicAdd(&s_nbig, 1u)] = pos;
            else if (dg >= 64) s_med[atomicAdd(&s_nmed, 1u)] = pos;
            else {
                uint32_t cnt = 0;
                for (int64_t e = beg; e < beg + dg; e++) edge(e, pos, cnt);
                if (cnt) atomicAdd(&d[pos], (unsigned long long)cnt);
            }
        }
        __syncthreads();
        const uint32_t nmed = s_nmed, nbig = s_nbig;
        for (uint32_t m = w; m < nmed; m += BLOCK / 64) {
            const uint32_t p = s_med[m], u = (uint32_t)order[p];
            const int64_t beg = row_ptr[u], end = row_ptr[u + 1];
            uint32_t cnt = 0;
            for (int64_t e = beg + lane; e < end; e += 64) edge(e, p, cnt);
            cnt = (uint32_t)wave_sum((uint64_t)cnt);
            if (lane == 0 && cnt) atomicAdd(&d[p], (unsigned long long)cnt);
        }
        for (uint32_t b = 0; b < nbig; b++) {
            if (threadIdx.x == 0) s_cnt = 0;
            __syncthreads();
            const uint32_t p = s_big[b], u = (uint32_t)order[p];
            const int64_t beg = row_ptr[u], end = row_ptr[u + 1];
            uint32_t cnt = 0;
            for (int64_t e = beg + threadIdx.x; e < end; e += BLOCK) edge(e, p, cnt);
            cnt = (uint32_t)wave_sum((uint64_t)cnt);
            if (lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
            __syncthreads();
            if (threadIdx.x == 0 && s_cnt) atomicAdd(&d[p], (unsigned long long)s_cnt);
        }
        __syncthreads(); // (the lists are refilled)
    }
}

// a prefix of the profile as a candidate: cut / den with den > 0 (den == 0: none), at position j
struct SwBest { uint64_t cut, den, vol; uint32_t j; };
// is a the better one?  cut_a * den_b < cut_b * den_a on the 128-bit products, ties to the smaller prefix
__device__ __forceinline__ bool sw_better(const SwBest &a, const SwBest &b) {
    if (!a.den) return false;
    if (!b.den) return true;
    const uint64_t lh = __umul64hi(a.cut, b.den), ll = a.cut * b.den, rh = __umul64hi(b.cut, a.den), rl = b.cut * a.den;
    if (lh != rh) return lh < rh;
    if (ll != rl) return ll < rl;
    return a.j < b.j;
}
__device__ __forceinline__ uint64_t sw_wave_incl(uint64_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint64_t x = __shfl_up(v, o); if (lane >= o) v += x; }
    return v;
}
// One workgroup per row of the chunk: cut = inclusive scan of the difference array, vol = inclusive scan of the degrees, both
// in place; den = min(vol, nnz - vol); the best prefix by sw_better.  grid = (rows of the chunk)
__global__ void __launch_bounds__(BLOCK) k_sweep_scan(const SweepRowDesc *rows, uint32_t r0, uint64_t *h_cut, uint64_t *h_vol, uint64_t hcap, uint64_t nnz,
                                                      SweepRowOut *out) {
    __shared__ uint64_t s_wc[BLOCK / 64], s_wv[BLOCK / 64];
    __shared__ uint64_t s_bc[BLOCK], s_bd[BLOCK], s_bv[BLOCK];
    __shared__ uint32_t s_bj[BLOCK];
    const SweepRowDesc rd = rows[r0 + blockIdx.x];
    const uint32_t L = (uint64_t)rd.hbase + rd.L <= hcap ? rd.L : 0;
    uint64_t *cutp = h_cut + rd.hbase, *volp = h_vol + rd.hbase;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t carry_c = 0, carry_v = 0;
    SwBest best{0, 0, 0, 0};
    for (uint32_t t0 = 0; t0 < L; t0 += BLOCK * SW_SCAN_ITEMS) {
        const uint32_t i0 = t0 + threadIdx.x * SW_SCAN_ITEMS;
        uint64_t cc[SW_SCAN_ITEMS], vv[SW_SCAN_ITEMS];
#pragma unroll
        for (int u = 0; u < SW_SCAN_ITEMS; u++) {
            const bool in = i0 + u < L;
            cc[u] = in ? cutp[i0 + u] : 0; vv[u] = in ? volp[i0 + u] : 0;
            if (u) { cc[u] += cc[u - 1]; vv[u] += vv[u - 1]; }
        }
        const uint64_t tc = cc[SW_SCAN_ITEMS - 1], tv = vv[SW_SCAN_ITEMS - 1];
        const uint64_t ic = sw_wave_incl(tc, lane), iv = sw_wave_incl(tv, lane);
        if (lane == 63) { s_wc[w] = ic; s_wv[w] = iv; }
        __syncthreads();
        uint64_t ec = carry_c + ic - tc, ev = carry_v + iv - tv, allc = 0, allv = 0;
#pragma unroll
        for (int x = 0; x < BLOCK / 64; x++) {
            if (x < w) { ec += s_wc[x]; ev += s_wv[x]; }
            allc += s_wc[x]; allv += s_wv[x];
        }
#pragma unroll
        for (int u = 0; u < SW_SCAN_ITEMS; u++)
            if (i0 + u < L) {
                const uint64_t c = ec + cc[u], v = ev + vv[u];
                cutp[i0 + u] = c; volp[i0 + u] = v;
                const SwBest cand{c, min(v, nnz - v), v, i0 + (uint32_t)u};
                if (sw_better(cand, best)) best = cand;
            }
        carry_c += allc; carry_v += allv;
        __syncthreads(); // (s_wc / s_wv are rewritten)
    }
    s_bc[threadIdx.x] = best.cut; s_bd[threadIdx.x] = best.den; s_bv[threadIdx.x] = best.vol; s_bj[threadIdx.x] = best.j;
    __syncthreads();
    for (int s = BLOCK / 2; s; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const SwBest a{s_bc[threadIdx.x], s_bd[threadIdx.x], s_bv[threadIdx.x], s_bj[threadIdx.x]};
            const SwBest b{s_bc[threadIdx.x + s], s_bd[threadIdx.x + s], s_bv[threadIdx.x + s], s_bj[threadIdx.x + s]};
            if (sw_better(b, a)) { s_bc[threadIdx.x] = b.cut; s_bd[threadIdx.x] = b.den; s_bv[threadIdx.x] = b.vol; s_bj[threadIdx.x] = b.j; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        SweepRowOut o;
        const bool any = s_bd[0] != 0;
        o.len = rd.len; o.best = any ? (int64_t)s_bj[0] + 1 : 0;
        o.cut = any ? s_bc[0] : 0; o.vol = any ? s_bv[0] : 0; o.den = s_bd[0];
        o.edges = carry_v;
        out[r0 + blockIdx.x] = o;
    }
}

// the one-entry profiles of dangling sources: order = the source, cut = vol = 0
__global__ void __launch_bounds__(BLOCK) k_sweep_single(uint32_t cnt, const int64_t *at, const int32_t *src, int32_t *h_ids, uint64_t *h_cut, uint64_t *h_vol, uint64_t hcap) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < cnt && (uint64_t)at[i] < hcap) { h_ids[at[i]] = src[i]; h_cut[at[i]] = 0; h_vol[at[i]] = 0; }
}

} // namespace fora
