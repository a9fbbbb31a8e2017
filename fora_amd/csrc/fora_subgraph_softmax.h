// fora_subgraph_softmax.h -- the kernels of EDGE SOFTMAX (fora_hip_subgraph_softmax, fora_hip_subgraph_softmax_bwd; the contract is
// in include/fora_hip_edge_softmax.h): the softmax of fora_softmax.h inside every GROUP of edges of the held subgraph, for every
// head, and its gradient.  A group is a row j of the subgraph -- the places sub_ptr[j] .. sub_ptr[j + 1] of sub_col -- or, by
// column, a column v -- the places in_pos[in_ptr[v] .. in_ptr[v + 1]) of its transposition.  scores, y, g and the outputs are
// [heads][edges] in the order of sub_col, so the value of head h at place e lies at h * edges + e whichever the grouping.
// Per head and group the bits are ROW SOFTMAX's on the group's sequence of values: the helpers below are those of fora_softmax.h
// with the place of an entry looked up once (`at`) where fora_softmax.h adds an offset, and smax_tree, smax_wave_max, smax_is_inf,
// smax_nan and exp_def are used as they stand.  Two paths, the same bits:
//   short  wave w of the grid owns group w: it reads the group's two offsets (wave-uniform), leaves if the group is empty or longer
//          than the cap, resolves the places of its entries ONCE -- by column one load of in_pos each -- and keeps them in registers
//          for all heads.  No host plan, no table, no LDS, no barrier.  A group of at most 64 entries -- nearly all of a
//          mini-batch's -- takes the branch in which a lane holds one value and SSM_HEADS = 4 heads are in flight, so the Horner
//          chains and the trees of four heads interleave; a longer one (up to 256) holds four values a lane, one head at a time,
//          whose four chains interleave as they do in k_softmax_short.  Every addition of the contract's tree is performed, those
//          of the +0.0 of the lanes past the group included: backward a term can be -0.0.
//   long   the 256-entry segments of the groups longer than the cap, one wave each, blockIdx.y the head: the three launches of
//          ROW SOFTMAX (two backward) with partials [heads][long segments].  The segment list (softmax_lists over the side's host
//          offsets) is made once per held subgraph, side and cap and kept on the device; a segment's `first` is a place in sub_col
//          by row and a position in in_pos by column.  A hub of 26 000 edges is 103 waves per head, not one.
// Nothing is fused: the file is compiled with -ffp-contract=off and every kernel says so again itself.
#pragma once
#include "fora_softmax.h"

namespace fora {

constexpr uint32_t SSM_WAVES = BLOCK / 64; // groups (short) or segments (long) per workgroup
constexpr int SSM_HEADS = 4;               // heads in flight in the branch len <= 64 of the short path

// the places in sub_col of the PER entries this lane holds of the entries [first, first + len) of a side
template <bool BYCOL, int PER>
__device__ __forceinline__ void ssm_places(const int64_t *__restrict__ pos, int64_t first, uint32_t len, uint32_t lane, uint64_t (&at)[PER]) {
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const uint32_t k = lane + 64u * (uint32_t)j;
        at[j] = 0;
        if (k < len) at[j] = BYCOL ? (uint64_t)pos[first + k] : (uint64_t)(first + k);
    }
}
// smax_load_x through the places: x of the lane's entries (sc: the head's slice), their maximum with a NaN read as +inf
template <typename TS, int PER>
__device__ __forceinline__ double ssm_load_x(const uint64_t (&at)[PER], uint32_t len, uint32_t lane, const TS *__restrict__ sc, double scale, double (&x)[PER]) {
#pragma clang fp contract(off)
    double m = smax_neg_inf();
#pragma unroll
    for (int j = 0; j < PER; j++) {
        x[j] = smax_neg_inf();
        if (lane + 64u * (uint32_t)j < len) {
            x[j] = (double)sc[at[j]] * scale;
            const double v = x[j] != x[j] ? -smax_neg_inf() : x[j];
            m = v > m ? v : m;
        }
    }
    return m;
}
// q_l of p = exp_def(x - m) over the lane's entries, p left in x; bad: the group is a NaN group, whatever is computed is dropped
template <int PER>
__device__ __forceinline__ double ssm_exp_q(uint32_t len, uint32_t lane, double m, bool bad, double (&x)[PER]) {
#pragma clang fp contract(off)
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        if (lane + 64u * (uint32_t)j < len) {
            const double t = x[j] - m;
            x[j] = exp_def(bad ? 0.0 : t);
            q = q + x[j];
        }
    }
    return q;
}
template <int PER>
__device__ __forceinline__ void ssm_store(const uint64_t (&at)[PER], uint32_t len, uint32_t lane, const double (&v)[PER], float *o32, double *o64) {
#pragma unroll
    for (int j = 0; j < PER; j++) {
        if (lane + 64u * (uint32_t)j < len) {
            if (o64) o64[at[j]] = v[j];
            if (o32) o32[at[j]] = (float)v[j];
        }
    }
}
// backward: y and g of the lane's entries and q_l of t = y * g
template <typename TY, typename TG, int PER>
__device__ __forceinline__ double ssm_bwd_q(const uint64_t (&at)[PER], uint32_t len, uint32_t lane, const TY *__restrict__ y, const TG *__restrict__ g,
                                            double (&yv)[PER], double (&gv)[PER]) {
#pragma clang fp contract(off)
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        yv[j] = gv[j] = 0.0;
        if (lane + 64u * (uint32_t)j < len) {
            yv[j] = (double)y[at[j]];
            gv[j] = (double)g[at[j]];
            const double t = yv[j] * gv[j];
            q = q + t;
        }
    }
    return q;
}
// dx = ((g - D) * y) * scale, left in yv
template <int PER>
__device__ __forceinline__ void ssm_bwd_dx(double D, double scale, double (&yv)[PER], const double (&gv)[PER]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const double a = gv[j] - D;
        const double b = a * yv[j];
        yv[j] = b * scale;
    }
}
__device__ __forceinline__ float *ssm_head(float *o, uint64_t off) { return o ? o + off : nullptr; }
__device__ __forceinline__ double *ssm_head(double *o, uint64_t off) { return o ? o + off : nullptr; }

// ---- the short path.  One group, every head, U heads in flight with PER values a lane each.  A head past the count is head
// heads - 1 again -- memory the wave reads anyway, no branch around a load -- and never stored or counted.
template <typename TS, int PER, int U>
__device__ __forceinline__ void ssm_group_fwd(const uint64_t (&at)[PER], uint32_t len, uint32_t lane, const TS *scores, uint64_t edges, uint32_t heads, double scale,
                                              float *out32, double *out64, uint32_t *nan_groups) {
#pragma clang fp contract(off)
    for (uint32_t h0 = 0; h0 < heads; h0 += (uint32_t)U) {
        double x[U][PER], m[U], q[U];
        uint64_t off[U];
        bool bad[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            off[u] = (uint64_t)min(h0 + (uint32_t)u, heads - 1u) * edges;
            m[u] = ssm_load_x<TS, PER>(at, len, lane, scores + off[u], scale, x[u]);
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
            if (h0 + (uint32_t)u >= heads) break;
#pragma unroll
            for (int j = 0; j < PER; j++) x[u][j] = bad[u] ? smax_nan() : x[u][j] / q[u];
            ssm_store<PER>(at, len, lane, x[u], ssm_head(out32, off[u]), ssm_head(out64, off[u]));
            if (bad[u] && lane == 0) atomicAdd(nan_groups, 1u);
        }
    }
}
template <typename TY, typename TG, int PER, int U>
__device__ __forceinline__ void ssm_group_bwd(const uint64_t (&at)[PER], uint32_t len, uint32_t lane, const TY *y, const TG *g, uint64_t edges, uint32_t heads, double scale,
                                              float *out32, double *out64) {
#pragma clang fp contract(off)
    for (uint32_t h0 = 0; h0 < heads; h0 += (uint32_t)U) {
        double yv[U][PER], gv[U][PER], q[U];
        uint64_t off[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            off[u] = (uint64_t)min(h0 + (uint32_t)u, heads - 1u) * edges;
            q[u] = ssm_bwd_q<TY, TG, PER>(at, len, lane, y + off[u], g + off[u], yv[u], gv[u]);
        }
#pragma unroll
        for (int u = 0; u < U; u++) q[u] = smax_tree(q[u]);
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (h0 + (uint32_t)u >= heads) break;
            ssm_bwd_dx<PER>(q[u], scale, yv[u], gv[u]);
            ssm_store<PER>(at, len, lane, yv[u], ssm_head(out32, off[u]), ssm_head(out64, off[u]));
        }
    }
}

// wave w of the grid and its group: first and len, or the whole wave leaves (past the last group, empty, longer than the cap).
// w is wave-uniform and the compiler is told so: the two offsets are scalar loads.
#define SSM_GROUP_PROLOGUE                                                                                                        \
    const uint32_t lane = threadIdx.x & 63u;                                                                                      \
    const uint64_t w = (uint64_t)blockIdx.x * SSM_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      \
    if (w >= ngroups) return;                                                                                                     \
    const int64_t first = ptr[w], count = ptr[w + 1] - first;                                                                     \
    if (count <= 0 || count > (int64_t)cap) return;                                                                               \
    const uint32_t len = (uint32_t)count;

// grid = ceil(ngroups / SSM_WAVES) workgroups of BLOCK threads.  ptr: sub_ptr, or in_ptr with pos = in_pos; cap <= PROP_SEG.
template <typename TS, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_softmax(const int64_t *__restrict__ ptr, uint32_t ngroups, uint32_t cap, const int64_t *__restrict__ pos,
                                                       const TS *scores, uint64_t edges, uint32_t heads, double scale, float *out32, double *out64, uint32_t *nan_groups) {
#pragma clang fp contract(off)
    SSM_GROUP_PROLOGUE
    if (len <= 64u) { // (uniform) a lane holds one value: the per-lane loop is gone, SSM_HEADS heads interleave
        uint64_t at[1];
        ssm_places<BYCOL, 1>(pos, first, len, lane, at);
        ssm_group_fwd<TS, 1, SSM_HEADS>(at, len, lane, scores, edges, heads, scale, out32, out64, nan_groups);
    } else {
        uint64_t at[SMAX_PER_LANE];
        ssm_places<BYCOL, (int)SMAX_PER_LANE>(pos, first, len, lane, at);
        ssm_group_fwd<TS, (int)SMAX_PER_LANE, 1>(at, len, lane, scores, edges, heads, scale, out32, out64, nan_groups);
    }
}
template <typename TY, typename TG, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_softmax_bwd(const int64_t *__restrict__ ptr, uint32_t ngroups, uint32_t cap, const int64_t *__restrict__ pos,
                                                           const TY *y, const TG *g, uint64_t edges, uint32_t heads, double scale, float *out32, double *out64) {
#pragma clang fp contract(off)
    SSM_GROUP_PROLOGUE
    if (len <= 64u) {
        uint64_t at[1];
        ssm_places<BYCOL, 1>(pos, first, len, lane, at);
        ssm_group_bwd<TY, TG, 1, SSM_HEADS>(at, len, lane, y, g, edges, heads, scale, out32, out64);
    } else {
        uint64_t at[SMAX_PER_LANE];
        ssm_places<BYCOL, (int)SMAX_PER_LANE>(pos, first, len, lane, at);
        ssm_group_bwd<TY, TG, (int)SMAX_PER_LANE, 1>(at, len, lane, y, g, edges, heads, scale, out32, out64);
    }
}
#undef SSM_GROUP_PROLOGUE

// ---- the long path.  grid = (ceil(nseg / SSM_WAVES), min(heads, 65535)): wave u of a grid row owns segment u of the long list
// for the heads blockIdx.y, blockIdx.y + gridDim.y, ...; seg_max and part are [heads][nseg], a head's row read through the slot
// and count of the segment's group exactly as ROW SOFTMAX reads its one row (smax_row_max, smax_row_sum).
#define SSM_SEG_PROLOGUE                                                                       \
    const uint32_t lane = threadIdx.x & 63u;                                                   \
    const uint64_t u = (uint64_t)blockIdx.x * SSM_WAVES + (threadIdx.x >> 6);                  \
    if (u >= nseg) return; /* (the whole wave) */                                              \
    const PropSeg sg = segs[u];                                                                \
    uint64_t at[SMAX_PER_LANE];                                                                \
    ssm_places<BYCOL, (int)SMAX_PER_LANE>(pos, sg.first, sg.len, lane, at);

template <typename TS, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_softmax_seg_max(const PropSeg *__restrict__ segs, uint64_t nseg, const int64_t *__restrict__ pos, const TS *scores, uint64_t edges,
                                                               uint32_t heads, double scale, double *seg_max) {
#pragma clang fp contract(off)
    SSM_SEG_PROLOGUE
    for (uint32_t h = blockIdx.y; h < heads; h += gridDim.y) {
        double x[SMAX_PER_LANE];
        const double m = smax_wave_max(ssm_load_x<TS, (int)SMAX_PER_LANE>(at, sg.len, lane, scores + (uint64_t)h * edges, scale, x));
        if (lane == 0) seg_max[(uint64_t)h * nseg + u] = m;
    }
}
template <typename TS, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_softmax_seg_sum(const PropSeg *__restrict__ segs, uint64_t nseg, const int64_t *__restrict__ pos, const TS *scores, uint64_t edges,
                                                               uint32_t heads, double scale, const double *seg_max, double *part) {
#pragma clang fp contract(off)
    SSM_SEG_PROLOGUE
    for (uint32_t h = blockIdx.y; h < heads; h += gridDim.y) {
        const double m = smax_row_max(sg, lane, seg_max + (uint64_t)h * nseg);
        if (smax_is_inf(m)) continue; // (a NaN group: k_sub_softmax_div writes it and reads no sum)
        double x[SMAX_PER_LANE];
        (void)ssm_load_x<TS, (int)SMAX_PER_LANE>(at, sg.len, lane, scores + (uint64_t)h * edges, scale, x);
        const double P = smax_tree(ssm_exp_q<(int)SMAX_PER_LANE>(sg.len, lane, m, false, x));
        if (lane == 0) part[(uint64_t)h * nseg + u] = P;
    }
}
template <typename TS, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_softmax_div(const PropSeg *__restrict__ segs, uint64_t nseg, const int64_t *__restrict__ pos, const TS *scores, uint64_t edges,
                                                           uint32_t heads, double scale, const double *seg_max, const double *part, float *out32, double *out64,
                                                           uint32_t *nan_groups) {
#pragma clang fp contract(off)
    SSM_SEG_PROLOGUE
    for (uint32_t h = blockIdx.y; h < heads; h += gridDim.y) {
        const uint64_t off = (uint64_t)h * edges;
        const double m = smax_row_max(sg, lane, seg_max + (uint64_t)h * nseg);
        const bool bad = smax_is_inf(m);
        double x[SMAX_PER_LANE];
        if (bad) {
#pragma unroll
            for (uint32_t j = 0; j < SMAX_PER_LANE; j++) x[j] = smax_nan();
            if (lane == 0 && u == sg.slot) atomicAdd(nan_groups, 1u); // (the group's first segment counts it)
        } else {
            const double S = smax_row_sum(sg, part + (uint64_t)h * nseg);
            (void)ssm_load_x<TS, (int)SMAX_PER_LANE>(at, sg.len, lane, scores + off, scale, x);
#pragma unroll
            for (uint32_t j = 0; j < SMAX_PER_LANE; j++) x[j] = exp_def(x[j] - m) / S; // (an entry past the segment: exp_def(-inf) = +0.0, never stored)
        }
        ssm_store<(int)SMAX_PER_LANE>(at, sg.len, lane, x, ssm_head(out32, off), ssm_head(out64, off));
    }
}
template <typename TY, typename TG, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_softmax_bwd_seg_sum(const PropSeg *__restrict__ segs, uint64_t nseg, const int64_t *__restrict__ pos, const TY *y, const TG *g,
                                                                   uint64_t edges, uint32_t heads, double *part) {
#pragma clang fp contract(off)
    SSM_SEG_PROLOGUE
    for (uint32_t h = blockIdx.y; h < heads; h += gridDim.y) {
        double yv[SMAX_PER_LANE], gv[SMAX_PER_LANE];
        const double P = smax_tree(ssm_bwd_q<TY, TG, (int)SMAX_PER_LANE>(at, sg.len, lane, y + (uint64_t)h * edges, g + (uint64_t)h * edges, yv, gv));
        if (lane == 0) part[(uint64_t)h * nseg + u] = P;
    }
}
template <typename TY, typename TG, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_softmax_bwd_div(const PropSeg *__restrict__ segs, uint64_t nseg, const int64_t *__restrict__ pos, const TY *y, const TG *g,
                                                               uint64_t edges, uint32_t heads, double scale, const double *part, float *out32, double *out64) {
#pragma clang fp contract(off)
    SSM_SEG_PROLOGUE
    for (uint32_t h = blockIdx.y; h < heads; h += gridDim.y) {
        const uint64_t off = (uint64_t)h * edges;
        double yv[SMAX_PER_LANE], gv[SMAX_PER_LANE];
        (void)ssm_bwd_q<TY, TG, (int)SMAX_PER_LANE>(at, sg.len, lane, y + off, g + off, yv, gv);
        ssm_bwd_dx<(int)SMAX_PER_LANE>(smax_row_sum(sg, part + (uint64_t)h * nseg), scale, yv, gv);
        ssm_store<(int)SMAX_PER_LANE>(at, sg.len, lane, yv, ssm_head(out32, off), ssm_head(out64, off));
    }
}
#undef SSM_SEG_PROLOGUE

} // namespace fora
