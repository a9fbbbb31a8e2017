// fora_prop.h -- the kernels of PROPAGATE (fora_hip_sparse_propagate; the contract is in include/fora_hip.h, the partition
// in fora_prop_plan.h): out[i][c] = sum over the entries e of held row i of w_e * H[id_e][c], every bit defined.
//   k_prop_gather   one lane group per (segment, column tile): P_s = the segment's terms added in entry order from +0.0,
//                   in f64 registers, stored to the chunk's partial-sum buffer part[slot][d];
//   k_prop_gather_t the same body over the transposition of the held result (PROPAGATE, TRANSPOSED; fora_propt.h builds it) when
//                   every weight is divided by its row's word sum; without that division the transposed product runs
//                   k_prop_gather itself, rows and columns swapped by the host;
//   k_prop_gather_vals  the same body with the caller's values as the weights (PROPAGATE WITH VALUES), over the held rows or
//                   over the transposition, where pos[p] (fora_propt.h) says which value entry p takes;
//   k_prop_combine  one lane per (row record, column): the row's P_s added in segment order, the carry of a row that a
//                   chunk cut, the normalisation, the stores with the output's pitch.
// Nothing here is fused: the file is compiled with -ffp-contract=off and the two kernels say so again themselves; there
// is no explicit fma.  The kernels take pointers and sizes, not Dev; BLOCK and fix2d come from fora_kernels.h.
#pragma once
#include "fora_kernels.h" // BLOCK, fix2d
#include "fora_narrow.h" // the element types, narrow_widen
#include "fora_prop_plan.h"

namespace fora {

constexpr int PROP_INFLIGHT = 4; // feature rows a lane group has in flight

// V adjacent columns of one feature row as they lie in memory: f32 one word per column, bf16 and f16 two columns per word,
// FP8 four (one column in the low end of the word when V == 1).  Loading and widening are apart on purpose: the kernel
// issues the loads of PROP_INFLIGHT rows first and widens to f64 only where it adds, so that no load waits for the one
// before it.  ET: the element type (fora_narrow.h), known where the kernel is compiled, since the layout hangs on it.
template <int ET, int V> struct PropRaw {
    static constexpr int PER = 4 / (int)elt_bytes(ET); // columns to a word
    static constexpr int W = V > PER ? V / PER : 1;
    uint32_t w[W];
};
// all V columns exist: one load of V elements -- the host chose V so that it is aligned (prop_geom)
template <int ET, int V>
__device__ __forceinline__ void prop_load_full(const void *feat, uint64_t off, PropRaw<ET, V> &r) {
    if constexpr (elt_bytes(ET) == 4) {
        const float *p = (const float *)feat + off;
        if constexpr (V == 4) { const uint4 x = *(const uint4 *)p; r.w[0] = x.x; r.w[1] = x.y; r.w[2] = x.z; r.w[3] = x.w; }
        else if constexpr (V == 2) { const uint2 x = *(const uint2 *)p; r.w[0] = x.x; r.w[1] = x.y; }
        else r.w[0] = __float_as_uint(p[0]);
    } else if constexpr (elt_bytes(ET) == 2) {
        const uint16_t *p = (const uint16_t *)feat + off;
        if constexpr (V == 8) { const uint4 x = *(const uint4 *)p; r.w[0] = x.x; r.w[1] = x.y; r.w[2] = x.z; r.w[3] = x.w; }
        else if constexpr (V == 4) { const uint2 x = *(const uint2 *)p; r.w[0] = x.x; r.w[1] = x.y; }
        else r.w[0] = p[0];
    } else {
        const uint8_t *p = (const uint8_t *)feat + off;
        if constexpr (V == 16) { const uint4 x = *(const uint4 *)p; r.w[0] = x.x; r.w[1] = x.y; r.w[2] = x.z; r.w[3] = x.w; }
        else if constexpr (V == 4) r.w[0] = *(const uint32_t *)p;
        else r.w[0] = p[0];
    }
}
// a tile's last lane: ncol < V columns exist, read one by one; the others stay 0 and are never stored
template <int ET, int V>
__device__ __forceinline__ void prop_load_tail(const void *feat, uint64_t off, uint32_t ncol, PropRaw<ET, V> &r) {
    if constexpr (elt_bytes(ET) == 4) {
        const float *p = (const float *)feat + off;
#pragma unroll
        for (int v = 0; v < V; v++) if ((uint32_t)v < ncol) r.w[v] = __float_as_uint(p[v]);
    } else if constexpr (elt_bytes(ET) == 2) {
        const uint16_t *p = (const uint16_t *)feat + off;
#pragma unroll
        for (int v = 0; v < V; v++) if ((uint32_t)v < ncol) r.w[v / 2] |= (uint32_t)p[v] << (16 * (v & 1));
    } else {
        const uint8_t *p = (const uint8_t *)feat + off;
#pragma unroll
        for (int v = 0; v < V; v++) if ((uint32_t)v < ncol) r.w[v / 4] |= (uint32_t)p[v] << (8 * (v & 3));
    }
}
// column v as a double: f32 widened, bf16 bits << 16 as f32 widened, a narrow type's code widened as fora_narrow.h says --
// all exact
template <int ET, int V>
__device__ __forceinline__ double prop_widen(const PropRaw<ET, V> &r, int v) {
    if constexpr (ET == ELT_F32) return (double)__uint_as_float(r.w[v]);
    else if constexpr (ET == ELT_BF16) {
        if constexpr (V == 1) return (double)__uint_as_float(r.w[0] << 16);
        else return (double)__uint_as_float((v & 1) ? (r.w[v / 2] & 0xFFFF0000u) : (r.w[v / 2] << 16));
    } else if constexpr (ET == ELT_F16) return (double)narrow_widen<ET>((r.w[v / 2] >> (16 * (v & 1))) & 0xFFFFu);
    else return (double)narrow_widen_byte<ET>(r.w[v / 4], v & 3);
}

// grid = (ceil(nseg / (segments per workgroup)), column tiles), BLOCK threads.  A wave holds 64 / G lane groups; group g of
// wave w of workgroup x owns segment (x * BLOCK / 64 + w) * (64 / G) + g and the columns [(y * G + gl) * V, ... + V) on its
// lane gl.  The group reads G entries of its segment at a time, one per lane -- ids and words read and the word converted
// once per column tile; G adjacent entries per load, so coalesced for wide groups, while with G == 1 (d <= V) every lane
// walks a segment of its own, 256 entries apart -- and hands them round with a shuffle inside the group.  The loads of up
// to PROP_INFLIGHT feature rows are issued before the first of them is widened and added; an entry past the group's
// count loads nothing.  The adds follow the entry order, so the partial sum does not depend on G, V or the grid.
// segsum (null: not wanted): the integer sum of the segment's words, by the groups of column tile 0.
// TNORM (the transposed product with FORA_PROP_NORMALIZE, k_prop_gather_t): the weight of an entry is its word divided by
// the word sum of the row it came from, rsum[id] -- one IEEE division per entry, made where the word is converted.
// WSRC (PROPAGATE WITH VALUES): where an entry's weight comes from -- PROP_W_FIX: its held word (the two kernels above, which
// compile to what they were before the parameter existed); PROP_W_VALUES: the caller's values[e], e the entry's place in the
// list (the forward product); PROP_W_POS: values[pos[p]], pos the held place of transposed entry p.  VAL64: values are f64,
// else f32 widened exactly.  With values no word is read and no word sum is made.  PROP_W_ONE: every weight is exactly 1.0 and
// nothing is read for it (SUBGRAPH PRODUCTS without values, fora_subgraph_prop.h).
enum : int { PROP_W_FIX = 0, PROP_W_VALUES = 1, PROP_W_POS = 2, PROP_W_ONE = 3 };
template <int ET, int V, bool TNORM, int WSRC = PROP_W_FIX, bool VAL64 = false>
__device__ __forceinline__ void prop_gather_body(const PropSeg *segs, uint64_t nseg, const int32_t *ids, const uint64_t *fix, const void *feat,
                                                 int64_t ldf, uint32_t d, uint32_t G, double *part, uint64_t *segsum, const uint64_t *rsum,
                                                 const void *values = nullptr, const int64_t *pos = nullptr) {
#pragma clang fp contract(off)
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
    uint64_t ssum = 0;
    for (uint32_t base = 0; base < len; base += G) {
        int32_t id_l = 0;
        double w_l = 0.0;
        if (base + gl < len) {
            if constexpr (WSRC == PROP_W_FIX) {
                const uint64_t f = fix[first + base + gl];
                id_l = ids[first + base + gl];
                ssum += f;
                w_l = fix2d(f);
                if constexpr (TNORM) w_l = w_l / fix2d(rsum[id_l]);
            } else if constexpr (WSRC == PROP_W_ONE) {
                id_l = ids[first + base + gl];
                w_l = 1.0;
            } else {
                id_l = ids[first + base + gl];
                int64_t at = first + base + gl;
                if constexpr (WSRC == PROP_W_POS) at = pos[at];
                if constexpr (VAL64) w_l = ((const double *)values)[at];
                else w_l = (double)((const float *)values)[at];
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
            if (ncol == (uint32_t)V) { // the full-lane / tail-lane choice stands outside the loop over the rows: the loads follow each other
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
    for (uint32_t o = G >> 1; o; o >>= 1) ssum += __shfl_xor(ssum, (int)o, (int)G);
    if (s < nseg) {
        if (segsum && gl == 0 && blockIdx.y == 0) segsum[slot] = ssum;
#pragma unroll
        for (int v = 0; v < V; v++)
            if ((uint32_t)v < ncol) part[(uint64_t)slot * d + c0 + (uint32_t)v] = acc[v];
    }
}
template <int ET, int V>
__global__ void __launch_bounds__(BLOCK) k_prop_gather(const PropSeg *segs, uint64_t nseg, const int32_t *ids, const uint64_t *fix, const void *feat,
                                                       int64_t ldf, uint32_t d, uint32_t G, double *part, uint64_t *segsum) {
    prop_gather_body<ET, V, false>(segs, nseg, ids, fix, feat, ldf, d, G, part, segsum, nullptr);
}
// the same over the transposition (ids: the rows of a column's entries, feat: the gradient), every weight divided by its row's
// word sum
template <int ET, int V>
__global__ void __launch_bounds__(BLOCK) k_prop_gather_t(const PropSeg *segs, uint64_t nseg, const int32_t *ids, const uint64_t *fix, const void *feat,
                                                         int64_t ldf, uint32_t d, uint32_t G, double *part, const uint64_t *rsum) {
    prop_gather_body<ET, V, true>(segs, nseg, ids, fix, feat, ldf, d, G, part, nullptr, rsum);
}

// PROPAGATE WITH VALUES: the same body with the caller's values as weights -- forward (pos null) and transposed
template <int ET, int V, bool POS, bool VAL64>
__global__ void __launch_bounds__(BLOCK) k_prop_gather_vals(const PropSeg *segs, uint64_t nseg, const int32_t *ids, const void *values, const int64_t *pos,
                                                            const void *feat, int64_t ldf, uint32_t d, uint32_t G, double *part) {
    prop_gather_body<ET, V, false, POS ? PROP_W_POS : PROP_W_VALUES, VAL64>(segs, nseg, ids, nullptr, feat, ldf, d, G, part, nullptr, nullptr, values, pos);
}

// One lane per (row record, column) of a chunk.  grid = (column blocks, record groups): with d >= BLOCK a workgroup takes
// BLOCK columns of one record, with d < BLOCK it takes rpb = BLOCK / d whole records (the host passes rpb; a 32-bit divide
// of the thread index, nothing wider); grid.y strides over the records.  carry_in / carry_out: d sums (scarry: one word
// sum) of the row that the chunk before cut / that this chunk cuts -- two buffers that swap from chunk to chunk, since the
// row that reads one and the row that writes one are different lanes.  segsum null: no normalisation.  out32 / out64:
// either may be null; each has its own pitch (a staged output is dense, the caller's device memory has the caller's ldo).
// MEAN (SUBGRAPH PRODUCTS, FORA_SUB_MEAN): the finished sum of row r divided once by its number of terms,
// mean_ptr[r + 1] - mean_ptr[r] (the records of such a plan have entries); without it mean_ptr is not read.
template <bool MEAN = false>
__global__ void __launch_bounds__(BLOCK) k_prop_combine(const PropRowRec *recs, uint64_t nrec, uint32_t d, uint32_t rpb, const double *part, const uint64_t *segsum,
                                                        const double *carry_in, double *carry_out, const uint64_t *scarry_in, uint64_t *scarry_out,
                                                        float *out32, int64_t ld32, double *out64, int64_t ld64, const int64_t *mean_ptr) {
#pragma clang fp contract(off)
    const uint32_t rl = rpb > 1 ? threadIdx.x / d : 0u;
    const uint32_t c = rpb > 1 ? threadIdx.x - rl * d : blockIdx.x * BLOCK + threadIdx.x;
    if (rl >= rpb || c >= d) return;
    for (uint64_t i = (uint64_t)blockIdx.y * rpb + rl; i < nrec; i += (uint64_t)gridDim.y * rpb) {
        const PropRowRec r = recs[i];
        double acc = 0.0;
        uint64_t S = 0;
        uint32_t k = 0;
        if (!(r.flags & PROP_FIRST)) { acc = carry_in[c]; if (segsum) S = scarry_in[0]; }
        else if (r.nseg) { acc = part[(uint64_t)r.slot0 * d + c]; if (segsum) S = segsum[r.slot0]; k = 1; }
        for (; k < r.nseg; k++) {
            acc = acc + part[(uint64_t)(r.slot0 + k) * d + c];
            if (segsum) S += segsum[r.slot0 + k];
        }
        if (!(r.flags & PROP_LAST)) {
            carry_out[c] = acc;
            if (segsum && c == 0) scarry_out[0] = S;
            continue;
        }
        if (segsum && S) acc = acc / fix2d(S);
        if constexpr (MEAN) {
            const int64_t terms = mean_ptr[r.row + 1] - mean_ptr[r.row];
            if (terms > 0) acc = acc / (double)terms;
        }
        if (out64) out64[(int64_t)r.row * ld64 + c] = acc;
        if (out32) out32[(int64_t)r.row * ld32 + c] = (float)acc;
    }
}

} // namespace fora
