// fora_subgraph_attn_bwd.h -- the fused kernels of EDGE ATTENTION, BACKWARD (fora_hip_subgraph_attention_bwd; the contract is in
// include/fora_hip_edge_attention_bwd.h).  Per head the gradients are a composition of contracts that exist -- dy = EDGE SCORES
// of (g, v); ds = EDGE SOFTMAX backward of (y, dy); dq = the SUBGRAPH PRODUCT along the forward call's grouping of k with ds;
// dk and dv = the product ACROSS it of q with ds and of g with y -- and the kernels here are built from the device functions
// that define those bits (sga_scores, sga_product, ssm_places, ssm_bwd_dx, ssm_store, the loads of fora_prop.h), so that
// nothing leaves f64 and no sum is added in another order.  The cut is k_sub_attn's: a wave owns one GROUP of at most
// PROP_SEG = 256 edges and a CHUNK of up to SGA_HEADS = 4 consecutive heads, unit u = group u / chunks, chunk u % chunks.
//   k_sub_attn_bwd     the along side, the mirror of k_sub_attn.  The group's ids staged once in LDS, the places of its entries
//                      in sub_col in registers.  dy by sga_scores over the group's row of g and the v rows of its ids, dv wide,
//                      to ysh[h - h0][place in the group].  D and ds in registers: y from the caller's array at h * edges +
//                      place (f32 or f64: a wave-uniform branch), dy from the lane's own places of LDS; a group of at most 64
//                      edges holds one value a lane with the chunk's heads in flight, a longer one four values a lane, one head
//                      at a time.  ds goes to the [heads][edges] buffer in EDGE order (only when dk is wanted) and back to the
//                      lane's own places of LDS; behind attn_wave_sync dq = sga_product over k, hc * d columns wide.
//   k_sub_attn_across  the across side, launched once for dk (values = the ds buffer, feat = q, w = d) and once for dv (values
//                      = y in the caller's type, feat = g, w = dv).  The other-end ids of the group staged in LDS, the chunk's
//                      values values[h * edges + place] staged in LDS as doubles (an f32 y widens exactly), then sga_product
//                      over the chunk's contiguous columns [h0 * w, (h0 + hc) * w) of feat: a row of q or g is read once per
//                      chunk of heads, not once per head.  A group of at most 256 edges is one segment of the product, so
//                      out = P_0: no partial sums, no combine.
//   k_sub_attn_y_gather  the longer groups by column: y of one head from edge order into position order, widened to f64, so
//                      that ROW SOFTMAX's segment kernels read it beside the dy k_prop_sddmm wrote in position order.
// dk and dv stay two launches: fused, a wave would hold two value arrays (2 x 4 x 256 doubles) beside the ids, 17 KB a wave and
// 68 KB a workgroup of four waves against the forward kernel's 36 KB, and the instantiations would be the product of the types
// of q and g (5 x 5 x widths) instead of their sum.
// An empty group writes its +0.0; a group longer than the cap leaves (the host runs it head by head through the steps' own
// kernels).  A wave's LDS is its own -- SGA_HEADS x 256 doubles and 256 ids, 9 KB -- and what one lane writes another reads only
// behind attn_wave_sync: no workgroup barrier.  Compiled with -ffp-contract=off, and every kernel says so again itself.
#pragma once
#include "fora_subgraph_attn.h" // sga_scores, sga_product, SGA_WAVES, SGA_HEADS

namespace fora {

// ssm_bwd_q with the two operands at places of their own: y of the lane's entries from the caller's array at `at`, dy from the
// head's row of the wave's LDS at the lane's own places; q_l of t = y * dy in the order of ssm_bwd_q
template <typename TY, int PER>
__device__ __forceinline__ double sgb_bwd_q(const uint64_t (&at)[PER], uint32_t len, uint32_t lane, const TY *__restrict__ y, const double *dysh, double (&yv)[PER],
                                            double (&gv)[PER]) {
#pragma clang fp contract(off)
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        yv[j] = gv[j] = 0.0;
        if (lane + 64u * (uint32_t)j < len) {
            yv[j] = (double)y[at[j]];
            gv[j] = dysh[lane + 64u * (uint32_t)j];
            const double t = yv[j] * gv[j];
            q = q + t;
        }
    }
    return q;
}

// the softmax backward of the chunk's heads, U of them in flight with PER values a lane each (ssm_group_bwd over the wave's
// LDS): ds to the ds buffer at the entries' places `at` (null: no across side reads it) and to the lane's own places of ysh,
// where it takes the place of dy -- no lane touches another's.  A head past the chunk is its last head again, never stored.
template <typename TY, int PER, int U>
__device__ __forceinline__ void sgb_softmax_bwd(double *ysh, const uint64_t (&at)[PER], uint32_t len, uint32_t lane, uint32_t h0, uint32_t hc, uint64_t edges,
                                                double scale, const TY *y, double *ds) {
#pragma clang fp contract(off)
    uint64_t self[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) self[j] = lane + 64u * (uint32_t)j;
    for (uint32_t b = 0; b < hc; b += (uint32_t)U) {
        double yv[U][PER], gv[U][PER], q[U];
        uint32_t h[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            h[u] = min(b + (uint32_t)u, hc - 1u);
            q[u] = sgb_bwd_q<TY, PER>(at, len, lane, y + (uint64_t)(h0 + h[u]) * edges, ysh + h[u] * PROP_SEG, yv[u], gv[u]);
        }
#pragma unroll
        for (int u = 0; u < U; u++) q[u] = smax_tree(q[u]);
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (b + (uint32_t)u >= hc) break;
            ssm_bwd_dx<PER>(q[u], scale, yv[u], gv[u]);
            ssm_store<PER>(at, len, lane, yv[u], nullptr, ssm_head(ds, (uint64_t)(h0 + h[u]) * edges));
            ssm_store<PER>(self, len, lane, yv[u], nullptr, ysh + h[u] * PROP_SEG);
        }
    }
}

// grid = ceil(ngroups * chunks / SGA_WAVES) workgroups of BLOCK threads, chunks = ceil(heads / SGA_HEADS).  ptr / ids / pos:
// sub_ptr, sub_col and null by row; in_ptr, in_row and in_pos by column.  g, v, k: the whole operands; head h reads the columns
// [h * dv, (h + 1) * dv) of g and v and [h * d, (h + 1) * d) of k.  lgv = log2 of the lane group that scores dv columns.  y:
// [heads][edges] in the order of sub_col, f64 when y_f64, else f32.  ds (null: dk is not wanted): [heads][edges] in that order.
// dq32 / dq64: ngroups x heads * d with their own pitches; both null: dq is not wanted and the product is skipped.  G_ET, V_ET:
// the types of g and v as sddmm_load takes them (types: sddmm_types() of the two, for ELT_ANY); K_ET: k's own type.
template <int G_ET, int V_ET, int K_ET, int V, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_attn_bwd(const int64_t *__restrict__ ptr, uint32_t ngroups, uint32_t cap, const int32_t *__restrict__ ids,
                                                        const int64_t *__restrict__ pos, uint32_t heads, uint32_t chunks, const void *g, int64_t ldg, const void *v,
                                                        int64_t ldv, const void *k, int64_t ldk, uint32_t d, uint32_t dv, uint32_t lgv, double scale, uint64_t edges,
                                                        const void *y, bool y_f64, double *ds, float *dq32, int64_t ld32, double *dq64, int64_t ld64, uint32_t types) {
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
    const uint32_t wc = hc * d;
    float *const o32 = dq32 ? dq32 + (int64_t)grp * ld32 + (uint64_t)h0 * d : nullptr;
    double *const o64 = dq64 ? dq64 + (int64_t)grp * ld64 + (uint64_t)h0 * d : nullptr;
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
    // ---- dy, each to its entry's place in the group
    sga_scores<G_ET, V_ET>(idsh, len, hc, g, grp * (uint64_t)ldg, v, ldv, (uint64_t)h0 * dv, dv, lgv, lane, types, ysh);
    attn_wave_sync();
    // ---- D and ds in registers; ds takes the place of dy
    if (len <= 64u) { // (uniform) a lane holds one value of a head, the chunk's heads interleave
        const uint64_t at1[1] = {at[0]};
        if (y_f64) sgb_softmax_bwd<double, 1, SGA_HEADS>(ysh, at1, len, lane, h0, hc, edges, scale, (const double *)y, ds);
        else sgb_softmax_bwd<float, 1, SGA_HEADS>(ysh, at1, len, lane, h0, hc, edges, scale, (const float *)y, ds);
    } else {
        if (y_f64) sgb_softmax_bwd<double, (int)SMAX_PER_LANE, 1>(ysh, at, len, lane, h0, hc, edges, scale, (const double *)y, ds);
        else sgb_softmax_bwd<float, (int)SMAX_PER_LANE, 1>(ysh, at, len, lane, h0, hc, edges, scale, (const float *)y, ds);
    }
    if (!o32 && !o64) return;
    attn_wave_sync();
    // ---- dq
    sga_product<K_ET, V>(ysh, idsh, len, k, ldk, (uint64_t)h0 * d, wc, d, 0u, lane, o32, o64);
}

// grid and units as k_sub_attn_bwd.  ptr / ids / pos: the ACROSS side's -- sub_ptr, sub_col and null when its groups are rows;
// in_ptr, in_row and in_pos when they are columns.  values: [heads][edges] in the order of sub_col, f64 when VAL64, else f32.
// feat: the whole operand, head h its columns [h * w, (h + 1) * w); out32 / out64: ngroups x heads * w with their own
// pitches, either may be null.
template <int ET, int V, bool VAL64, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_attn_across(const int64_t *__restrict__ ptr, uint32_t ngroups, uint32_t cap, const int32_t *__restrict__ ids,
                                                           const int64_t *__restrict__ pos, uint32_t heads, uint32_t chunks, const void *values, uint64_t edges,
                                                           const void *feat, int64_t ldf, uint32_t w, float *out32, int64_t ld32, double *out64, int64_t ld64) {
#pragma clang fp contract(off)
    __shared__ double sh_y[SGA_WAVES][SGA_HEADS * PROP_SEG];
    __shared__ int32_t sh_id[SGA_WAVES][PROP_SEG];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t u = (uint64_t)blockIdx.x * SGA_WAVES + wave;
    const uint64_t grp = u / chunks;
    if (grp >= ngroups) return; // (the whole wave; there is no workgroup barrier below)
    const uint32_t h0 = (uint32_t)(u % chunks) * (uint32_t)SGA_HEADS, hc = min((uint32_t)SGA_HEADS, heads - h0);
    const int64_t first = ptr[grp], count = ptr[grp + 1] - first; // (scalar loads)
    if (count > (int64_t)cap) return;                             // (the long path's)
    const uint32_t wc = hc * w;
    float *const o32 = out32 ? out32 + (int64_t)grp * ld32 + (uint64_t)h0 * w : nullptr;
    double *const o64 = out64 ? out64 + (int64_t)grp * ld64 + (uint64_t)h0 * w : nullptr;
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
    for (uint32_t h = 0; h < hc; h++) { // the chunk's values, each to its entry's place in the group
        const uint64_t off = (uint64_t)(h0 + h) * edges;
#pragma unroll
        for (uint32_t j = 0; j < SMAX_PER_LANE; j++) {
            if (lane + 64u * j < len) {
                if constexpr (VAL64) ysh[h * PROP_SEG + lane + 64u * j] = ((const double *)values)[off + at[j]];
                else ysh[h * PROP_SEG + lane + 64u * j] = (double)((const float *)values)[off + at[j]];
            }
        }
    }
    attn_wave_sync();
    sga_product<ET, V>(ysh, idsh, len, feat, ldf, (uint64_t)h0 * w, wc, w, 0u, lane, o32, o64);
}

// The groups of the long path by column: y of one head lies in edge order; this gathers it into position order, widened,
// o[p] = (double)y[in_pos[p]] -- the inverse of k_sub_attn_y_places.  rows: one PropSeg per long group (first, len); y points at
// the head's first element.  grid = (ceil(longest / BLOCK) capped, min(nrow, 65535)).
template <typename TY>
__global__ void __launch_bounds__(BLOCK) k_sub_attn_y_gather(const PropSeg *rows, uint64_t nrow, const int64_t *__restrict__ pos, const TY *y, double *o) {
    for (uint64_t i = blockIdx.y; i < nrow; i += gridDim.y) {
        const PropSeg r = rows[i];
        for (uint32_t k = blockIdx.x * BLOCK + threadIdx.x; k < r.len; k += gridDim.x * BLOCK) o[r.first + k] = (double)y[pos[r.first + k]];
    }
}

} // namespace fora
