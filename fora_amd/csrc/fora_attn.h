// fora_attn.h -- the fused kernel of ATTENTION (fora_hip_sparse_attention; the contract is in include/fora_hip.h): for a held
// row of at most PROP_SEG = 256 entries and one head, SCORES (SDDMM), ROW SOFTMAX and PROPAGATE WITH VALUES in one wave, with
// nothing leaving the CU between the steps and every bit what the three calls chained through f64 give.
//   scores   sddmm_scores (fora_sddmm.h), the loop k_prop_sddmm runs: lane groups over the columns of the head's slice of q
//            and k, four entries in flight, the merged trees.  A finished score goes to the wave's LDS, at its entry's place.
//   softmax  the device functions of fora_softmax.h on registers: lane l owns the places l, l + 64, l + 128, l + 192 as in
//            k_softmax_short -- x = score * scale, the wave's maximum with a NaN riding as +inf, exp_def, the 64 lane sums and
//            the six-step tree, one division.  y goes back to LDS (and to the y outputs when they are wanted).
//   product  lanes over the head's dv columns of v, V adjacent ones per lane (the host chose V as prop_geom does), a tile of
//            64 * V columns at a time; the entries one after the other in held order, acc = acc + y_e * v[id_e][c] from +0.0,
//            y_e and id_e read from LDS by every lane, PROP_INFLIGHT rows of v in flight.  The row is one segment: out = P_0.
// A NaN row (fora_softmax.h) is written, not computed: the quiet NaN to its y and to its dv outputs, and lane 0 counts it.
// An empty row writes +0.0 to its dv outputs.  A wave's LDS is its own -- 256 doubles and 256 ids, 3 KB -- and what one lane
// writes another reads only behind a wave-wide fence: no workgroup barrier, a wave with no work just leaves.
// Nothing is fused: the file is compiled with -ffp-contract=off and the kernel says so again itself.
#pragma once
#include "fora_prop.h"    // PropRaw, prop_load_full / _tail, prop_widen, PROP_INFLIGHT
#include "fora_sddmm.h"   // sddmm_scores
#include "fora_softmax.h" // the smax_* functions
#include "fora_attn_plan.h"

namespace fora {

constexpr uint32_t ATTN_ROWS = BLOCK / 64; // (row, head) pairs per workgroup, one wave each

// LDS written by some lanes of the wave, read by others: the writes are done and visible before any lane goes on
__device__ __forceinline__ void attn_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the product of one (row, head): o32 / o64 point at the head's first output column of the row (either may be null)
template <int ET, int V>
__device__ __forceinline__ void attn_product(const double *ysh, const int32_t *idsh, uint32_t len, const void *v, int64_t ldv, uint64_t vcol, uint32_t dv,
                                             uint32_t lane, float *o32, double *o64) {
#pragma clang fp contract(off)
    for (uint32_t c0 = lane * (uint32_t)V; c0 < dv; c0 += 64u * (uint32_t)V) {
        const uint32_t ncol = min((uint32_t)V, dv - c0);
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
                w[u] = ysh[from];
#pragma unroll
                for (int j = 0; j < PropRaw<ET, V>::W; j++) raw[u].w[j] = 0;
            }
            if (ncol == (uint32_t)V) { // (as in prop_gather_body: the choice stands outside the loop over the rows)
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
#pragma unroll
        for (int i = 0; i < V; i++) {
            if ((uint32_t)i < ncol) {
                if (o64) o64[c0 + (uint32_t)i] = acc[i];
                if (o32) o32[c0 + (uint32_t)i] = (float)acc[i];
            }
        }
    }
}

// grid = ceil(nrow * heads / ATTN_ROWS) workgroups of BLOCK threads.  Wave u of the grid owns head u % heads of row u / heads
// of the list (adjacent waves share a row of q).  q, k, v: the whole operands; head j reads the columns [j * d, (j + 1) * d) of
// q and k and [j * dv, (j + 1) * dv) of v.  lg = log2 of the lane group of the scores.  out32 / out64: nq x heads * dv with
// their own pitches, either may be null; y32 / y64: [heads][entries], both may be null.  Q_ET, K_ET: the types of the two
// one-element-per-lane operands as sddmm_load takes them (types: sddmm_types() of the two, for ELT_ANY); V_ET: v's own type.
template <int Q_ET, int K_ET, int V_ET, int V>
__global__ void __launch_bounds__(BLOCK) k_attn_short(const PropSeg *rows, uint64_t nrow, uint32_t heads, const int32_t *ids, const void *q, int64_t ldq,
                                                      const void *k, int64_t ldk, const void *v, int64_t ldv, uint32_t d, uint32_t dv, uint32_t lg,
                                                      double scale, uint64_t entries, float *out32, int64_t ld32, double *out64, int64_t ld64,
                                                      float *y32, double *y64, uint32_t *nan_rows, uint32_t types) {
#pragma clang fp contract(off)
    __shared__ double sh_y[ATTN_ROWS][PROP_SEG];
    __shared__ int32_t sh_id[ATTN_ROWS][PROP_SEG];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t u = (uint64_t)blockIdx.x * ATTN_ROWS + wave;
    if (u >= nrow * heads) return; // (the whole wave)
    const uint32_t head = (uint32_t)(u % heads);
    PropSeg sg = rows[u / heads];
    sg.len = min(sg.len, PROP_SEG); // (the host lists no longer row; a wave's LDS holds this many)
    double *const ysh = sh_y[wave];
    int32_t *const idsh = sh_id[wave];
    float *const o32 = out32 ? out32 + (int64_t)sg.row * ld32 + (uint64_t)head * dv : nullptr;
    double *const o64 = out64 ? out64 + (int64_t)sg.row * ld64 + (uint64_t)head * dv : nullptr;
    if (!sg.len) { // an empty row: +0.0
        for (uint32_t c = lane; c < dv; c += 64u) {
            if (o64) o64[c] = 0.0;
            if (o32) o32[c] = 0.0f;
        }
        return;
    }
    // ---- scores, each to its entry's place
#pragma unroll
    for (uint32_t j = 0; j < SMAX_PER_LANE; j++)
        if (lane + 64u * j < sg.len) idsh[lane + 64u * j] = ids[sg.first + lane + 64u * j];
    sddmm_scores<Q_ET, K_ET>(ids + sg.first, sg.len, q, (uint64_t)(uint32_t)sg.row * (uint64_t)ldq + (uint64_t)head * d, k, ldk, (uint64_t)head * d, d, lg, lane, types,
                                 [=](uint32_t e, double s) { ysh[e] = s; });
    attn_wave_sync();
    // ---- softmax in registers
    PropSeg rel = sg; // the row as a segment of the LDS array
    rel.first = 0;
    PropSeg ysg = sg; // and of the head's y
    ysg.first = (int64_t)((uint64_t)head * entries) + sg.first;
    double x[SMAX_PER_LANE];
    const double m = smax_wave_max(smax_load_x(rel, lane, (const double *)ysh, scale, x));
    if (smax_is_inf(m)) { // (the whole wave: a NaN entry, +inf, or nothing above -inf)
#pragma unroll
        for (uint32_t j = 0; j < SMAX_PER_LANE; j++) x[j] = smax_nan();
        smax_store(ysg, lane, x, y32, y64);
        for (uint32_t c = lane; c < dv; c += 64u) {
            if (o64) o64[c] = smax_nan();
            if (o32) o32[c] = (float)smax_nan();
        }
        if (lane == 0) atomicAdd(nan_rows, 1u);
        return;
    }
    const double S = smax_exp_sum(rel, lane, m, x);
#pragma unroll
    for (uint32_t j = 0; j < SMAX_PER_LANE; j++) x[j] = x[j] / S;
    smax_store(ysg, lane, x, y32, y64);
    attn_wave_sync(); // (every lane has read its scores before y takes their place)
    smax_store(rel, lane, x, nullptr, ysh);
    attn_wave_sync();
    // ---- the product
    attn_product<V_ET, V>(ysh, idsh, sg.len, v, ldv, (uint64_t)head * dv, dv, lane, o32, o64);
}

// The longer rows go through the existing kernels, whose products define no NaN payload: this one rewrites the dv outputs of
// every (row, head) that ROW SOFTMAX wrote as NaN -- y of the row's first entry says so -- with the quiet NaN.  rows: one
// PropSeg per longer row (first, row); y: the head's y in f64; out32 / out64 point at the head's first column.
// grid = (ceil(dv / BLOCK), min(nrow, 65535)).
__global__ void __launch_bounds__(BLOCK) k_attn_nan_rows(const PropSeg *rows, uint64_t nrow, const double *y, uint32_t dv, float *out32, int64_t ld32,
                                                         double *out64, int64_t ld64) {
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= dv) return;
    for (uint64_t i = blockIdx.y; i < nrow; i += gridDim.y) {
        const PropSeg r = rows[i];
        const double y0 = y[r.first];
        if (y0 == y0) continue;
        if (out64) out64[(int64_t)r.row * ld64 + c] = smax_nan();
        if (out32) out32[(int64_t)r.row * ld32 + c] = (float)smax_nan();
    }
}

} // namespace fora
