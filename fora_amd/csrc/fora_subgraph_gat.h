// fora_subgraph_gat.h -- the kernels of EDGE GAT (fora_hip_subgraph_gat, fora_hip_subgraph_gat_bwd; the contract is in
// include/fora_hip_edge_gat.h): attention over the edges of the held subgraph with the ADDITIVE score of a graph attention
// network, z_e = el[row(e)] + er[sub_col[e]], s_e = LeakyReLU(z_e), one scalar per node and head on either end.  Per head every
// bit is the composition the contract words -- one f64 addition, one f64 multiplication and a select, then EDGE SOFTMAX and the
// SUBGRAPH PRODUCT with the f64 probabilities -- and the kernels are built from the device functions that define those bits
// (sga_softmax, sga_product, sga_scores, sgb_bwd_q, ssm_bwd_dx, ssm_places, ssm_store), so no sum is added in another order.
// A score here is a 4-byte-or-less load and an addition, not a d-long dot product: there are no lane groups and no trees, the
// scoring step all but vanishes and a layer is bound by the rows of v.  The cut is k_sub_attn's -- a wave owns one GROUP of at
// most PROP_SEG = 256 edges (a row of sub_ptr; by column the positions in_ptr[u] .. in_ptr[u + 1] of the transposition) and a
// CHUNK of up to SGA_HEADS = 4 consecutive heads, unit u = group u / chunks, chunk u % chunks -- and so is the wave's LDS.
//   lane map   entry k of the group belongs to lane k % 64, its place j = k / 64 (four places a lane at most): the layout in
//              which ssm_load_x reads a head's row of the wave's LDS.  A lane scores its own places, so the scores reach the
//              softmax without an exchange, and dz of the backward pass is written where its lane computed it.
//   operands   z is read at the edge's row and column under both groupings; the grouping decides which end is the GROUP's.
//              The group-side operand (el by row, er by column) is wave-uniform: hc scalars, loaded once.  The other end's is
//              one contiguous run of the chunk's hc scalars at the id of the entry -- a row of it comes in once per chunk.  The
//              f64 addition commutes, so el + er and er + el are the same bits.  The element types of el and er are read at
//              run time (sddmm_load<ELT_ANY>: one element per lane, nothing about the layout hangs on the type); only v's type,
//              whose loads are vectors, is compiled in.
//   k_sub_gat          ids to LDS; scores at the lane's own places of ysh[h - h0]; sga_softmax (y to the y outputs and back to
//                      LDS); behind attn_wave_sync sga_product over the chunk's contiguous columns of v.
//   k_sub_gat_bwd      the along side.  dy by sga_scores over the group's row of g and the v rows of the ids, dv wide; D and ds
//                      in registers as in k_sub_attn_bwd; z computed again from el and er, dz = ds or ds * slope, to the
//                      [heads][edges] dz buffer in EDGE order (only when the across sum is wanted) and to the lane's own places
//                      of LDS; behind attn_wave_sync lane h of the chunk adds the group's dz left to right from +0.0 -- the
//                      product of a ones column with dz as values, a group being one segment of it.
//   k_sub_gat_across   the across sum of dz.  A wave owns one group of the OPPOSITE side and all heads: it stages the group's dz
//                      of as many heads as its LDS takes (1028 doubles / the group's length, at least SGA_HEADS), places along
//                      the lanes so that a head's reads coalesce, and lane h adds head h's in the across order from +0.0.  It
//                      reads no feature matrix.  A head's row of LDS is len | 1 doubles long: lanes that walk their rows side
//                      by side then hit different banks.
//   k_gat_seg          the longer groups, one head: a thread per entry of a 256-entry segment of the along side's plan, the
//                      score in position order (forward) or dz in place of ds (backward).
//   k_gat_ones         the ones column the longer groups' sums of dz multiply, [nc] f32.
// dv of the backward pass is k_sub_attn_across as it stands, values = y and feat = g.
// An empty group writes its +0.0; a group longer than the cap leaves (the host runs it head by head through the steps' own
// kernels).  A wave's LDS is its own and what one lane writes another reads only behind attn_wave_sync: no workgroup barrier.
// Compiled with -ffp-contract=off, and every kernel says so again itself.
#pragma once
#include "fora_subgraph_attn_bwd.h" // sga_softmax, sga_product, sga_scores, sgb_bwd_q, SGA_WAVES, SGA_HEADS

namespace fora {

constexpr uint32_t GAT_X_LDS = (uint32_t)SGA_HEADS * (PROP_SEG + 1u); // doubles of a wave of k_sub_gat_across: SGA_HEADS rows of 256 | 1

__device__ __forceinline__ double gat_load(const void *m, uint64_t at, int rt) { return (double)__uint_as_float(sddmm_load<ELT_ANY>(m, at, rt)); }
// the score of a pre-activation: z itself from +-0.0 up, z * slope below and for a NaN
__device__ __forceinline__ double gat_leaky(double z, double slope) {
#pragma clang fp contract(off)
    const double t = z * slope;
    return z >= 0.0 ? z : t;
}
// its gradient: ds where z was passed on, ds * slope where it was multiplied
__device__ __forceinline__ double gat_leaky_bwd(double z, double ds, double slope) {
#pragma clang fp contract(off)
    const double t = ds * slope;
    return z >= 0.0 ? ds : t;
}

// z of the lane's places of the chunk's heads: zs[h][j] for entry lane + 64 j.  gs: the group's hc scalars (wave-uniform);
// os: the other end's operand, col0 = h0; a head past the chunk and a place past the group are never read
template <int PER>
__device__ __forceinline__ void gat_z(const int32_t *idsh, uint32_t len, uint32_t lane, uint32_t hc, const double (&gs)[SGA_HEADS], const void *os, int64_t ldos,
                                      uint64_t col0, int o_rt, double (&zs)[SGA_HEADS][PER]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const uint32_t k = lane + 64u * (uint32_t)j;
        const uint64_t at = k < len ? (uint64_t)(uint32_t)idsh[k] * (uint64_t)ldos + col0 : 0ull;
#pragma unroll
        for (int h = 0; h < SGA_HEADS; h++) {
            zs[h][j] = 0.0;
            if (k < len && (uint32_t)h < hc) zs[h][j] = gs[h] + gat_load(os, at + (uint32_t)h, o_rt);
        }
    }
}

// The unit of a wave of k_sub_gat and k_sub_gat_bwd, as k_sub_attn cuts it: lane, wave, grp, h0, hc, first, len, the outputs
// o32 / o64 of the chunk (W columns a head), ysh, idsh, the places `at` and the staged ids; an empty group has written its
// +0.0 and left, a group past the last or longer than the cap has left.  No lane is past a workgroup barrier: there is none.
#define GAT_UNIT_PROLOGUE(W, out32, out64)                                                                                            \
    __shared__ double sh_y[SGA_WAVES][SGA_HEADS * PROP_SEG];                                                                          \
    __shared__ int32_t sh_id[SGA_WAVES][PROP_SEG];                                                                                    \
    const uint32_t lane = threadIdx.x & 63u;                                                                                          \
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));                                          \
    const uint64_t u = (uint64_t)blockIdx.x * SGA_WAVES + wave;                                                                       \
    const uint64_t grp = u / chunks;                                                                                                  \
    if (grp >= ngroups) return;                                                                                                       \
    const uint32_t h0 = (uint32_t)(u % chunks) * (uint32_t)SGA_HEADS, hc = min((uint32_t)SGA_HEADS, heads - h0);                      \
    const int64_t first = ptr[grp], count = ptr[grp + 1] - first;                                                                     \
    if (count > (int64_t)cap) return;                                                                                                 \
    const uint32_t wc = hc * (uint32_t)(W);                                                                                           \
    float *const o32 = out32 ? out32 + (int64_t)grp * ld32 + (uint64_t)h0 * (uint32_t)(W) : nullptr;                                  \
    double *const o64 = out64 ? out64 + (int64_t)grp * ld64 + (uint64_t)h0 * (uint32_t)(W) : nullptr;                                 \
    if (count <= 0) {                                                                                                                 \
        for (uint32_t c = lane; c < wc; c += 64u) {                                                                                   \
            if (o64) o64[c] = 0.0;                                                                                                    \
            if (o32) o32[c] = 0.0f;                                                                                                   \
        }                                                                                                                             \
        return;                                                                                                                       \
    }                                                                                                                                 \
    const uint32_t len = (uint32_t)count;                                                                                             \
    double *const ysh = sh_y[wave];                                                                                                   \
    int32_t *const idsh = sh_id[wave];                                                                                                \
    uint64_t at[SMAX_PER_LANE];                                                                                                       \
    ssm_places<BYCOL, (int)SMAX_PER_LANE>(pos, first, len, lane, at);                                                                 \
    _Pragma("unroll") for (uint32_t j = 0; j < SMAX_PER_LANE; j++)                                                                    \
        if (lane + 64u * j < len) idsh[lane + 64u * j] = ids[first + lane + 64u * j];                                                 \
    double gsv[SGA_HEADS];                                                                                                            \
    _Pragma("unroll") for (int h = 0; h < SGA_HEADS; h++)                                                                             \
        gsv[h] = gat_load(gs, grp * (uint64_t)ldgs + h0 + min((uint32_t)h, hc - 1u), (int)(types & 0xFFu));

// the chunk's scores to the lane's own places of ysh: a lane reads back only what it wrote itself
template <int PER>
__device__ __forceinline__ void gat_scores(double *ysh, const int32_t *idsh, uint32_t len, uint32_t lane, uint32_t hc, const double (&gs)[SGA_HEADS], const void *os,
                                           int64_t ldos, uint64_t col0, int o_rt, double slope) {
#pragma clang fp contract(off)
    double zs[SGA_HEADS][PER];
    gat_z<PER>(idsh, len, lane, hc, gs, os, ldos, col0, o_rt, zs);
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const uint32_t k = lane + 64u * (uint32_t)j;
#pragma unroll
        for (int h = 0; h < SGA_HEADS; h++)
            if (k < len && (uint32_t)h < hc) ysh[(uint32_t)h * PROP_SEG + k] = gat_leaky(zs[h][j], slope);
    }
}

// grid = ceil(ngroups * chunks / SGA_WAVES) workgroups of BLOCK threads, chunks = ceil(heads / SGA_HEADS).  ptr / ids / pos:
// sub_ptr, sub_col and null by row; in_ptr, in_row and in_pos by column.  gs: the operand read at the group (el by row, er by
// column), os: the one read at the id; both [nc, heads] at their pitches, types = sddmm_types() of the two.  v: the whole
// operand, head h its columns [h * dv, (h + 1) * dv).  out32 / out64: ngroups x heads * dv with their own pitches, either may
// be null; y32 / y64: [heads][edges], both may be null.
template <int V_ET, int V, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_gat(const int64_t *__restrict__ ptr, uint32_t ngroups, uint32_t cap, const int32_t *__restrict__ ids,
                                                   const int64_t *__restrict__ pos, uint32_t heads, uint32_t chunks, const void *gs, int64_t ldgs, const void *os,
                                                   int64_t ldos, const void *v, int64_t ldv, uint32_t dv, double slope, uint64_t edges, float *out32, int64_t ld32,
                                                   double *out64, int64_t ld64, float *y32, double *y64, uint32_t *nan_pairs, uint32_t types) {
#pragma clang fp contract(off)
    GAT_UNIT_PROLOGUE(dv, out32, out64)
    const int o_rt = (int)(types >> 8);
    uint32_t nan_heads;
    if (len <= 64u) { // (uniform) a lane holds one value of a head, the chunk's heads interleave
        const uint64_t at1[1] = {at[0]};
        gat_scores<1>(ysh, idsh, len, lane, hc, gsv, os, ldos, h0, o_rt, slope);
        nan_heads = sga_softmax<1, SGA_HEADS>(ysh, at1, len, lane, h0, hc, edges, 1.0, y32, y64);
    } else {
        gat_scores<(int)SMAX_PER_LANE>(ysh, idsh, len, lane, hc, gsv, os, ldos, h0, o_rt, slope);
        nan_heads = sga_softmax<(int)SMAX_PER_LANE, 1>(ysh, at, len, lane, h0, hc, edges, 1.0, y32, y64);
    }
    if (nan_heads && lane == 0) atomicAdd(nan_pairs, (uint32_t)__popc(nan_heads));
    attn_wave_sync(); // (the ids and y of every lane, before the product reads them)
    sga_product<V_ET, V>(ysh, idsh, len, v, ldv, (uint64_t)h0 * dv, wc, dv, nan_heads, lane, o32, o64);
}

// sgb_softmax_bwd with the LeakyReLU behind it: ds in registers, dz = ds or ds * slope by the z of the entry, to the dz
// buffer at the entries' places `at` (null: no across sum reads it) and to the lane's own places of ysh in place of dy
template <typename TY, int PER, int U>
__device__ __forceinline__ void gat_softmax_bwd(double *ysh, const int32_t *idsh, const uint64_t (&at)[PER], uint32_t len, uint32_t lane, uint32_t h0, uint32_t hc,
                                                uint64_t edges, const TY *y, const double (&gs)[SGA_HEADS], const void *os, int64_t ldos, int o_rt, double slope,
                                                double *dz) {
#pragma clang fp contract(off)
    static_assert(U == 1 || U == SGA_HEADS, "one head at a time, or the chunk's");
    uint64_t self[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) self[j] = lane + 64u * (uint32_t)j;
    double zs[SGA_HEADS][PER];
    gat_z<PER>(idsh, len, lane, hc, gs, os, ldos, h0, o_rt, zs);
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
            ssm_bwd_dx<PER>(q[u], 1.0, yv[u], gv[u]);
#pragma unroll
            for (int j = 0; j < PER; j++) {
                double z = zs[0][j]; // (the head is b + u: a compile-time index when U is the chunk, a select when U is 1)
#pragma unroll
                for (int hh = 1; hh < SGA_HEADS; hh++) z = h[u] == (uint32_t)hh ? zs[hh][j] : z;
                yv[u][j] = gat_leaky_bwd(z, yv[u][j], slope);
            }
            ssm_store<PER>(at, len, lane, yv[u], nullptr, ssm_head(dz, (uint64_t)(h0 + h[u]) * edges));
            ssm_store<PER>(self, len, lane, yv[u], nullptr, ysh + h[u] * PROP_SEG);
        }
    }
}

// grid and units as k_sub_gat.  gs, os, types: as there.  g, v: the whole operands, head h their columns [h * dv, (h + 1) * dv);
// lgv = log2 of the lane group that scores dv columns, gv_types = sddmm_types() of the two for ELT_ANY.  y: [heads][edges] in
// the order of sub_col, f64 when y_f64, else f32.  dz (null: no across sum is wanted): [heads][edges] in that order.  dg32 /
// dg64: the gradient of gs, ngroups x heads with their own pitches; both null: it is not wanted and its sum is skipped.
template <int G_ET, int V_ET, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_gat_bwd(const int64_t *__restrict__ ptr, uint32_t ngroups, uint32_t cap, const int32_t *__restrict__ ids,
                                                       const int64_t *__restrict__ pos, uint32_t heads, uint32_t chunks, const void *gs, int64_t ldgs, const void *os,
                                                       int64_t ldos, const void *g, int64_t ldg, const void *v, int64_t ldv, uint32_t dv, uint32_t lgv, double slope,
                                                       uint64_t edges, const void *y, bool y_f64, double *dz, float *dg32, int64_t ld32, double *dg64, int64_t ld64,
                                                       uint32_t types, uint32_t gv_types) {
#pragma clang fp contract(off)
    GAT_UNIT_PROLOGUE(1u, dg32, dg64)
    const int o_rt = (int)(types >> 8);
    attn_wave_sync();
    // ---- dy, each to its entry's place in the group
    sga_scores<G_ET, V_ET>(idsh, len, hc, g, grp * (uint64_t)ldg, v, ldv, (uint64_t)h0 * dv, dv, lgv, lane, gv_types, ysh);
    attn_wave_sync();
    // ---- D, ds and dz in registers; dz takes the place of dy
    if (len <= 64u) { // (uniform) a lane holds one value of a head, the chunk's heads interleave
        const uint64_t at1[1] = {at[0]};
        if (y_f64) gat_softmax_bwd<double, 1, SGA_HEADS>(ysh, idsh, at1, len, lane, h0, hc, edges, (const double *)y, gsv, os, ldos, o_rt, slope, dz);
        else gat_softmax_bwd<float, 1, SGA_HEADS>(ysh, idsh, at1, len, lane, h0, hc, edges, (const float *)y, gsv, os, ldos, o_rt, slope, dz);
    } else {
        if (y_f64) gat_softmax_bwd<double, (int)SMAX_PER_LANE, 1>(ysh, idsh, at, len, lane, h0, hc, edges, (const double *)y, gsv, os, ldos, o_rt, slope, dz);
        else gat_softmax_bwd<float, (int)SMAX_PER_LANE, 1>(ysh, idsh, at, len, lane, h0, hc, edges, (const float *)y, gsv, os, ldos, o_rt, slope, dz);
    }
    if (!o32 && !o64) return;
    attn_wave_sync();
    // ---- the gradient of the group's scalars: lane h adds head h0 + h's dz in group order
    if (lane < wc) {
        const double *const row = ysh + lane * PROP_SEG;
        double acc = 0.0;
        for (uint32_t k = 0; k < len; k++) acc = acc + row[k];
        if (o64) o64[lane] = acc;
        if (o32) o32[lane] = (float)acc;
    }
}

// grid = ceil(ngroups / SGA_WAVES) workgroups of BLOCK threads: a wave per group of the ACROSS side, all heads.  ptr / pos:
// sub_ptr and null when its groups are rows; in_ptr and in_pos when they are columns.  dz: [heads][edges] in the order of
// sub_col.  out32 / out64: ngroups x heads with their own pitches, either may be null.
template <bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_gat_across(const int64_t *__restrict__ ptr, uint32_t ngroups, uint32_t cap, const int64_t *__restrict__ pos,
                                                          uint32_t heads, const double *__restrict__ dz, uint64_t edges, float *out32, int64_t ld32, double *out64,
                                                          int64_t ld64) {
#pragma clang fp contract(off)
    __shared__ double sh_z[SGA_WAVES][GAT_X_LDS];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t grp = (uint64_t)blockIdx.x * SGA_WAVES + wave;
    if (grp >= ngroups) return; // (the whole wave; there is no workgroup barrier below)
    const int64_t first = ptr[grp], count = ptr[grp + 1] - first; // (scalar loads)
    if (count > (int64_t)cap) return;                             // (the long path's)
    float *const o32 = out32 ? out32 + (int64_t)grp * ld32 : nullptr;
    double *const o64 = out64 ? out64 + (int64_t)grp * ld64 : nullptr;
    if (count <= 0) { // an empty group: +0.0, whatever the cap
        for (uint32_t h = lane; h < heads; h += 64u) {
            if (o64) o64[h] = 0.0;
            if (o32) o32[h] = 0.0f;
        }
        return;
    }
    const uint32_t len = (uint32_t)count; // (at most PROP_SEG: the host clamps the cap)
    double *const zsh = sh_z[wave];
    uint64_t at[SMAX_PER_LANE];
    ssm_places<BYCOL, (int)SMAX_PER_LANE>(pos, first, len, lane, at);
    const uint32_t pitch = len | 1u, pass = min(64u, GAT_X_LDS / pitch); // heads a pass: at least SGA_HEADS, a lane each
    for (uint32_t hb = 0; hb < heads; hb += pass) {
        const uint32_t n = min(pass, heads - hb);
        for (uint32_t h = 0; h < n; h++) {
            const double *const src = dz + (uint64_t)(hb + h) * edges;
#pragma unroll
            for (uint32_t j = 0; j < SMAX_PER_LANE; j++)
                if (lane + 64u * j < len) zsh[h * pitch + lane + 64u * j] = src[at[j]];
        }
        attn_wave_sync();
        if (lane < n) {
            const double *const row = zsh + lane * pitch;
            double acc = 0.0;
            for (uint32_t k = 0; k < len; k++) acc = acc + row[k];
            if (o64) o64[hb + lane] = acc;
            if (o32) o32[hb + lane] = (float)acc;
        }
        attn_wave_sync(); // (every lane has read its row before the next pass writes)
    }
}

// The longer groups, one head: segment s of the along side's plan is blockIdx.x + i * gridDim.x, thread k its entry k.  gs, os:
// the head's column of the two operands; x: the head's per-entry array in the along side's position order -- forward the score
// is written to it, backward (BWD) it holds ds and dz takes its place.  grid = min(nseg, 2^31 - 1) workgroups of PROP_SEG threads.
template <bool BWD>
__global__ void __launch_bounds__(BLOCK) k_gat_seg(const PropSeg *__restrict__ segs, uint64_t nseg, const int32_t *__restrict__ ids, const void *gs, int64_t ldgs,
                                                   const void *os, int64_t ldos, uint32_t types, double slope, double *x) {
#pragma clang fp contract(off)
    static_assert(BLOCK == (int)PROP_SEG, "a thread per entry of a segment");
    for (uint64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const PropSeg sg = segs[s];
        if (threadIdx.x >= sg.len) continue;
        const int64_t p = sg.first + threadIdx.x;
        const double z = gat_load(gs, (uint64_t)(uint32_t)sg.row * (uint64_t)ldgs, (int)(types & 0xFFu)) +
                         gat_load(os, (uint64_t)(uint32_t)ids[p] * (uint64_t)ldos, (int)(types >> 8));
        x[p] = BWD ? gat_leaky_bwd(z, x[p], slope) : gat_leaky(z, slope);
    }
}

__global__ void __launch_bounds__(BLOCK) k_gat_ones(float *o, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) o[i] = 1.0f;
}

#undef GAT_UNIT_PROLOGUE

} // namespace fora
