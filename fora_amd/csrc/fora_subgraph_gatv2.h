// fora_subgraph_gatv2.h -- the kernels of EDGE GATV2 (fora_hip_subgraph_gatv2; the contract is in include/fora_hip_edge_gatv2.h):
// attention over the edges of the held subgraph with the score of GATv2, the non-linearity INSIDE the sum,
//   s_e[h] = sum over c of att[h, c] * LeakyReLU(xl[row(e), h d + c] + xr[sub_col[e], h d + c]),
// then EDGE SOFTMAX and the SUBGRAPH PRODUCT with the f64 probabilities.  Per element one f64 addition, gat_leaky, one f64
// multiplication (it rounds) and one f64 addition into the running sum q_l of lane l = c mod 64; the tree of SCORES ends the sum.
// The cut is k_sub_attn's -- a wave owns one GROUP of at most PROP_SEG = 256 edges and a CHUNK of up to SGA_HEADS = 4 consecutive
// heads -- and the softmax and the product are sga_softmax and sga_product as they stand.  What is this file's own is the scoring:
//   items      the (edge, head) pairs of the chunk, p = k * hc + h, side by side as in sga_scores: a lane group of 2^lg >= d lanes
//              (64 from d = 33 up) per pair, SDDMM_INFLIGHT = 4 pairs in flight, the four trees merged.  Groups side by side hold
//              the chunk's heads of ONE edge, so a row of the gathered operand comes in once for the chunk, as whole lines.
//   operands   three per column where the dot product has two: the GATHERED end (xr[id] by row, xl[id] by column), the GROUP's
//              own row of the other operand, and att[h].  The f64 addition commutes, so xl + xr and xr + xl are the same bits:
//              the host hands the kernel (gs, os) = (xl, xr) by row and (xr, xl) by column, as EDGE GAT does.
//   staging    the last two are the same for every edge of the group: the chunk's hc * d elements of each are widened to f32
//              (exact for all five types) and staged ONCE per unit in the wave's LDS, gs at [0, hc d), att behind it.  A lane then
//              reads its column's pair from LDS where it would issue two more global loads per pair and round.  The bound is
//              GV2_STAGE = 512 elements a chunk (hc * d <= 512: four heads of 128 columns) -- 4 KB more than k_sub_attn's 9 KB a
//              wave, 52 KB a workgroup, three workgroups in a CU's 160 KB.  A wider chunk reads the two in place through the
//              cache (wave-uniform choice; the bits are the same).
//   types      xl, xr and att are read at run time (sddmm_load<ELT_ANY>: one element per lane, nothing about the layout hangs
//              on the type); only v's type, whose loads are vectors, is compiled in: 5 types x 3 widths x 2 groupings = 30
//              instantiations of k_sub_gatv2, where the gathered type compiled in as in sga_scores would make 90.
//   k_sub_gatv2   ids and the staged rows to LDS; the scores to ysh[h - h0][place]; sga_softmax; sga_product.
//   k_gatv2_seg   the longer groups, one head: a wave scores SDDMM_SUB = 64 entries of a 256-entry segment of the along side's
//                 plan with the same function (hc = 1, the ids read in place), the score to position order.
// No matrix instructions: a d-long sum with a select inside and a fixed f64 order.  A wave's LDS is its own and what one lane
// writes another reads only behind attn_wave_sync: no workgroup barrier.  Compiled with -ffp-contract=off, and every kernel says
// so again itself.
#pragma once
#include "fora_subgraph_gat.h" // gat_leaky; sga_softmax, sga_product, SGA_WAVES, SGA_HEADS

namespace fora {

constexpr uint32_t GV2_STAGE = 512; // elements of gs, and of att, that a wave stages: hc * d at most

// the run-time types of gs, os and att in one kernel argument
constexpr uint32_t gatv2_types(int gs_type, int os_type, int att_type) { return (uint32_t)gs_type | (uint32_t)os_type << 8 | (uint32_t)att_type << 16; }

// the chunk's hc * d elements of the group's row of gs (grow: its first element of the chunk) and of att (arow: the first
// element of the chunk's first head, pitch ldatt) as f32 into stg[0, hc d) and stg[GV2_STAGE, GV2_STAGE + hc d)
__device__ __forceinline__ void gatv2_stage(float *stg, const void *gs, uint64_t grow, const void *att, uint64_t arow, int64_t ldatt, uint32_t hc, uint32_t d,
                                            uint32_t lane, uint32_t types) {
    const int g_rt = (int)(types & 0xFFu), a_rt = (int)(types >> 16 & 0xFFu);
    for (uint32_t i = lane; i < hc * d; i += 64u) {
        const uint32_t h = i / d, c = i - h * d;
        stg[i] = __uint_as_float(sddmm_load<ELT_ANY>(gs, grow + i, g_rt));
        stg[GV2_STAGE + i] = __uint_as_float(sddmm_load<ELT_ANY>(att, arow + (uint64_t)h * (uint64_t)ldatt + c, a_rt));
    }
}

// The scores of the pairs p = k * hc + h, k < len, h < hc, by one whole wave: sink(k, h, s) is called once per pair on the lane
// that ends up with its score.  ids: the len ids of the gathered rows (LDS or global).  stg: the staged rows (gatv2_stage), or
// null: gs and att are read in place at grow and arow.  os: the gathered operand, ocol the chunk's first column of it.  Every
// lane runs every round; a pair past the count is scored as pair 0 again and dropped.
template <typename Sink>
__device__ __forceinline__ void gatv2_scores(const int32_t *ids, uint32_t len, uint32_t hc, const float *stg, const void *gs, uint64_t grow, const void *att,
                                             uint64_t arow, int64_t ldatt, const void *os, int64_t ldos, uint64_t ocol, uint32_t d, uint32_t lg, uint32_t lane,
                                             uint32_t types, double slope, Sink &&sink) {
#pragma clang fp contract(off)
    const int g_rt = (int)(types & 0xFFu), o_rt = (int)(types >> 8 & 0xFFu), a_rt = (int)(types >> 16 & 0xFFu);
    const uint32_t G = 1u << lg;
    const uint32_t gl = lane & (G - 1u), grp = lane >> lg, ngrp = 64u >> lg;
    const uint32_t np = len * hc; // (at most 256 * SGA_HEADS)
    for (uint32_t p0 = 0; p0 < np; p0 += ngrp * SDDMM_INFLIGHT) {
        uint64_t oat[SDDMM_INFLIGHT];
        uint32_t ek[SDDMM_INFLIGHT], hd[SDDMM_INFLIGHT];
        bool valid[SDDMM_INFLIGHT];
        double s[SDDMM_INFLIGHT];
#pragma unroll
        for (int u = 0; u < SDDMM_INFLIGHT; u++) {
            const uint32_t p = p0 + (uint32_t)u * ngrp + grp;
            valid[u] = p < np;
            ek[u] = valid[u] ? (hc == 1u ? p : p / hc) : 0u;
            hd[u] = valid[u] ? p - ek[u] * hc : 0u;
            oat[u] = (uint64_t)(uint32_t)ids[ek[u]] * (uint64_t)ldos + ocol + (uint64_t)hd[u] * d;
            s[u] = 0.0;
        }
        for (uint32_t c = gl; c < d; c += 64u) {
            uint32_t ro[SDDMM_INFLIGHT];
            float rg[SDDMM_INFLIGHT], ra[SDDMM_INFLIGHT];
#pragma unroll
            for (int u = 0; u < SDDMM_INFLIGHT; u++) ro[u] = sddmm_load<ELT_ANY>(os, oat[u] + c, o_rt);
            if (stg) { // (uniform) the group's row and att from the wave's LDS
#pragma unroll
                for (int u = 0; u < SDDMM_INFLIGHT; u++) {
                    rg[u] = stg[hd[u] * d + c];
                    ra[u] = stg[GV2_STAGE + hd[u] * d + c];
                }
            } else {
#pragma unroll
                for (int u = 0; u < SDDMM_INFLIGHT; u++) {
                    rg[u] = __uint_as_float(sddmm_load<ELT_ANY>(gs, grow + (uint64_t)hd[u] * d + c, g_rt));
                    ra[u] = __uint_as_float(sddmm_load<ELT_ANY>(att, arow + (uint64_t)hd[u] * (uint64_t)ldatt + c, a_rt));
                }
            }
#pragma unroll
            for (int u = 0; u < SDDMM_INFLIGHT; u++) {
                const double z = (double)rg[u] + (double)__uint_as_float(ro[u]);
                const double t = (double)ra[u] * gat_leaky(z, slope);
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
                const uint32_t k = up2 ? (up1 ? ek[3] : ek[2]) : (up1 ? ek[1] : ek[0]);
                const uint32_t h = up2 ? (up1 ? hd[3] : hd[2]) : (up1 ? hd[1] : hd[0]);
                if (ok) sink(k, h, t);
            }
        } else {
            if (G == 2u) {
#pragma unroll
                for (int u = 0; u < SDDMM_INFLIGHT; u++) s[u] = s[u] + __shfl_down(s[u], 1u, 2);
            }
            if (gl == 0) {
#pragma unroll
                for (int u = 0; u < SDDMM_INFLIGHT; u++)
                    if (valid[u]) sink(ek[u], hd[u], s[u]);
            }
        }
    }
}

// grid = ceil(ngroups * chunks / SGA_WAVES) workgroups of BLOCK threads, chunks = ceil(heads / SGA_HEADS).  ptr / ids / pos:
// sub_ptr, sub_col and null by row; in_ptr, in_row and in_pos by column.  gs: the operand read at the group (xl by row, xr by
// column), os: the one read at the id, both [nc, heads * d]; att: [heads, d]; types = gatv2_types() of the three.  lg = log2 of
// the lane group of the scores.  v: the whole operand, head h its columns [h * dv, (h + 1) * dv).  out32 / out64: ngroups x
// heads * dv with their own pitches, either may be null; y32 / y64: [heads][edges], both may be null.
template <int V_ET, int V, bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_gatv2(const int64_t *__restrict__ ptr, uint32_t ngroups, uint32_t cap, const int32_t *__restrict__ ids,
                                                     const int64_t *__restrict__ pos, uint32_t heads, uint32_t chunks, const void *gs, int64_t ldgs, const void *os,
                                                     int64_t ldos, const void *att, int64_t ldatt, const void *v, int64_t ldv, uint32_t d, uint32_t dv, uint32_t lg,
                                                     double slope, uint64_t edges, float *out32, int64_t ld32, double *out64, int64_t ld64, float *y32, double *y64,
                                                     uint32_t *nan_pairs, uint32_t types) {
#pragma clang fp contract(off)
    __shared__ double sh_y[SGA_WAVES][SGA_HEADS * PROP_SEG];
    __shared__ int32_t sh_id[SGA_WAVES][PROP_SEG];
    __shared__ float sh_st[SGA_WAVES][2 * GV2_STAGE];
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
    const uint64_t grow = grp * (uint64_t)ldgs + (uint64_t)h0 * d, arow = (uint64_t)h0 * (uint64_t)ldatt;
    const float *const stg = (uint64_t)hc * d <= GV2_STAGE ? sh_st[wave] : nullptr; // (uniform) a wider chunk reads gs and att in place
    if (stg) gatv2_stage(sh_st[wave], gs, grow, att, arow, ldatt, hc, d, lane, types);
    attn_wave_sync();
    gatv2_scores(idsh, len, hc, stg, gs, grow, att, arow, ldatt, os, ldos, (uint64_t)h0 * d, d, lg, lane, types, slope,
                 [=](uint32_t k, uint32_t h, double s) { ysh[h * PROP_SEG + k] = s; });
    attn_wave_sync();
    uint32_t nan_heads;
    if (len <= 64u) { // (uniform) a lane holds one value of a head, the chunk's heads interleave
        const uint64_t at1[1] = {at[0]};
        nan_heads = sga_softmax<1, SGA_HEADS>(ysh, at1, len, lane, h0, hc, edges, 1.0, y32, y64);
    } else {
        nan_heads = sga_softmax<(int)SMAX_PER_LANE, 1>(ysh, at, len, lane, h0, hc, edges, 1.0, y32, y64);
    }
    if (nan_heads && lane == 0) atomicAdd(nan_pairs, (uint32_t)__popc(nan_heads));
    attn_wave_sync(); // (the ids and y of every lane, before the product reads them)
    sga_product<V_ET, V>(ysh, idsh, len, v, ldv, (uint64_t)h0 * dv, wc, dv, nan_heads, lane, o32, o64);
}

// The longer groups, one head.  grid = ceil(nseg * SDDMM_UNITS / (BLOCK / 64)) workgroups of BLOCK threads: wave u of the grid
// owns the entries [sub * SDDMM_SUB, ...) of segment u / SDDMM_UNITS of the along side's plan, sub = u % SDDMM_UNITS, as in
// k_prop_sddmm.  gs, os: the head's first column of the two operands; att: the head's row; x: the head's scores in the along
// side's position order.  The group's row and att are staged as in k_sub_gatv2 while d <= GV2_STAGE.
__global__ void __launch_bounds__(BLOCK) k_gatv2_seg(const PropSeg *__restrict__ segs, uint64_t nseg, const int32_t *__restrict__ ids, const void *gs, int64_t ldgs,
                                                     const void *os, int64_t ldos, const void *att, uint32_t d, uint32_t lg, uint32_t types, double slope, double *x) {
#pragma clang fp contract(off)
    __shared__ float sh_st[BLOCK / 64][2 * GV2_STAGE];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t unit = (uint64_t)blockIdx.x * (BLOCK / 64) + wave;
    const uint64_t s = unit / SDDMM_UNITS;
    const uint32_t lo = (uint32_t)(unit % SDDMM_UNITS) * SDDMM_SUB;
    if (s >= nseg) return; // (the whole wave)
    const PropSeg sg = segs[s];
    if (lo >= sg.len) return;
    const uint32_t cnt = min(SDDMM_SUB, sg.len - lo);
    const int64_t e0 = sg.first + lo;
    const uint64_t grow = (uint64_t)(uint32_t)sg.row * (uint64_t)ldgs;
    const float *const stg = d <= GV2_STAGE ? sh_st[wave] : nullptr;
    if (stg) gatv2_stage(sh_st[wave], gs, grow, att, 0ull, 0, 1u, d, lane, types);
    attn_wave_sync();
    gatv2_scores(ids + e0, cnt, 1u, stg, gs, grow, att, 0ull, 0, os, ldos, 0ull, d, lg, lane, types, slope, [=](uint32_t k, uint32_t, double sc) { x[e0 + k] = sc; });
}

} // namespace fora
