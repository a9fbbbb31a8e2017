// fora_subgraph_gatv2_bwd.h -- the kernels of EDGE GATV2, BACKWARD (fora_hip_subgraph_gatv2_bwd; the contract is in
// include/fora_hip_edge_gatv2_bwd.h): the gradients of GATv2 attention over the held subgraph with respect to xl, xr, att and v.
// dy, ds and dv are EDGE GAT, BACKWARD's, built from the same device functions (sga_scores, sgb_softmax_bwd, k_sub_attn_across).
// What is this file's own is the way back through the score: per edge e, head h and column c
//   u = xl[row(e)] + xr[col(e)],  du = ds_e * (u >= 0 ? att : att * slope),  a = ds_e * LeakyReLU(u),
// du summed over the edges of a node on either side (d xl, d xr), a over all edges (d att) -- sums ACROSS EDGES, PER COLUMN, in
// the fixed order of the SUBGRAPH PRODUCT.  The forward kernel's split (a lane group per (edge, head) pair, trees across columns)
// cannot serve them; the split here is a LANE PER COLUMN with the edges serial:
//   gatv2_accumulate   the shared device function of both sides.  A wave has one group's (or one 256-entry segment's) ids and its
//                      ds; lane l owns the columns i = l + 64 j of the chunk's hc * d, GV2_COLS = 8 of them a pass (the chunk of
//                      four heads of 128 columns is one pass; a wider one takes further passes over the entries).  The group's own
//                      row of its operand and att are the SAME for every entry of a column: the lane reads its columns' elements
//                      once, widens them and keeps them in registers with att * slope beside them -- what the forward kernel has
//                      to stage in LDS because there a column changes lanes, here stays where it is used.  The wave then walks the
//                      entries in order, GV2_FLIGHT = 4 entries' gathered rows in flight (the loads are coalesced across the lanes
//                      and a row comes in as whole lines once per chunk); the additions stay in entry order, from +0.0.  No
//                      shuffles, no trees.
//   k_sub_gatv2_bwd    the along side: k_sub_gat_bwd's cut and prologue -- one group of at most 256 edges and a chunk of up to
//                      four heads per wave; dy by sga_scores, D and ds in registers (sgb_softmax_bwd), ds to the [heads][edges]
//                      f64 buffer in edge order (only when the across gradient is wanted) and to the lane's own places of LDS;
//                      behind attn_wave_sync gatv2_accumulate writes the gradient row of the group's operand and, when d att is
//                      wanted, the group's row P_g of the [nc, heads * d] f64 scratch.
//   k_sub_gatv2_across the across side: a wave per group of the OPPOSITE side and chunk; ids and places as k_sub_gat_across, ds
//                      gathered from the buffer into LDS, gatv2_accumulate with the operand roles swapped.  It reads no
//                      [edges, d] intermediate: the only per-edge buffer of the call is ds, heads * edges doubles.
//   k_gatv2_bwd_seg    the longer groups of either side: a wave per (256-entry segment of that side's plan, chunk) runs
//                      gatv2_accumulate with the ids and ds read in place and writes the segment's partial rows;
//   k_gatv2_bwd_join   adds a group's segment partials in order, acc = P_0, acc = acc + P_s, into the gradient row and into P_g.
//   k_gatv2_datt       the two-level column sum of P: threads across the heads * d columns, the tiles of GV2_TILE = 256
//                      consecutive groups in parallel, then the same kernel once over the tile sums.
// No matrix instructions: every sum here has a select inside and a fixed f64 order of additions.  A wave's LDS is its own and
// what one lane writes another reads only behind attn_wave_sync: no workgroup barrier.  Compiled with -ffp-contract=off, and every
// kernel says so again itself.
#pragma once
#include "fora_subgraph_gatv2.h" // gatv2_types; gat_leaky; sga_scores, sgb_softmax_bwd, SGA_WAVES, SGA_HEADS

namespace fora {

constexpr uint32_t GV2_COLS = 8;   // columns a lane owns in one pass over the entries: 64 * 8 = GV2_STAGE columns a pass
constexpr uint32_t GV2_FLIGHT = 4; // entries whose gathered rows are in flight
constexpr uint32_t GV2_TILE = 256; // FORA_GATV2_DATT_TILE of the contract: consecutive groups whose P rows one tile sum adds
static_assert(64u * GV2_COLS == GV2_STAGE, "a pass covers the forward kernel's staged chunk");

// The sums of one group or segment over the chunk's wc = hc * d columns.  ids: the len ids of the gathered rows (LDS or
// global); ds(h, k): ds of entry k and head h0 + h.  gs: the operand read at the group's own node, grow the first element of
// the chunk in its row; att: arow the first element of the chunk's first head, pitch ldatt; os: the gathered operand, ocol the
// chunk's first column of it; types = gatv2_types(gs, os, att).  o32 / o64: the chunk's first element of the row that takes
// the sum of du (either may be null); p64: of the row that takes the sum of a (null: not wanted, WITH_P false).
template <bool WITH_P, typename Ds>
__device__ __forceinline__ void gatv2_accumulate(const int32_t *ids, uint32_t len, Ds &&ds, const void *gs, uint64_t grow, const void *att, uint64_t arow, int64_t ldatt,
                                                 const void *os, int64_t ldos, uint64_t ocol, uint32_t wc, uint32_t d, uint32_t lane, uint32_t types, double slope,
                                                 float *o32, double *o64, double *p64) {
#pragma clang fp contract(off)
    const int g_rt = (int)(types & 0xFFu), o_rt = (int)(types >> 8 & 0xFFu), a_rt = (int)(types >> 16 & 0xFFu);
    for (uint32_t c0 = 0; c0 < wc; c0 += 64u * GV2_COLS) { // (uniform) one pass while hc * d <= GV2_STAGE
        const uint32_t nj = min(GV2_COLS, (wc - c0 + 63u) / 64u); // (uniform) the column slots of a lane this pass fills: one while hc * d <= 64
        uint32_t col[GV2_COLS], hd[GV2_COLS];
        double gv[GV2_COLS], av[GV2_COLS], as[GV2_COLS], dx[GV2_COLS], pa[GV2_COLS];
#pragma unroll
        for (uint32_t j = 0; j < GV2_COLS; j++) {
            const uint32_t i = c0 + lane + 64u * j;
            col[j] = i < wc ? i : 0u; // a column past the chunk is column 0 again, never stored
            hd[j] = col[j] / d;
            gv[j] = av[j] = 0.0;
            if (j < nj) {
                gv[j] = (double)__uint_as_float(sddmm_load<ELT_ANY>(gs, grow + col[j], g_rt));
                av[j] = (double)__uint_as_float(sddmm_load<ELT_ANY>(att, arow + (uint64_t)hd[j] * (uint64_t)ldatt + (col[j] - hd[j] * d), a_rt));
            }
            as[j] = av[j] * slope; // w of a multiplied entry: the contract's one multiplication, the same for every entry
            dx[j] = pa[j] = 0.0;
        }
        for (uint32_t k0 = 0; k0 < len; k0 += GV2_FLIGHT) {
            uint32_t ro[GV2_FLIGHT][GV2_COLS];
#pragma unroll
            for (uint32_t f = 0; f < GV2_FLIGHT; f++) { // an entry past the group is its last one again, never added
                const uint64_t at = (uint64_t)(uint32_t)ids[min(k0 + f, len - 1u)] * (uint64_t)ldos + ocol;
#pragma unroll
                for (uint32_t j = 0; j < GV2_COLS; j++) ro[f][j] = j < nj ? sddmm_load<ELT_ANY>(os, at + col[j], o_rt) : 0u;
            }
#pragma unroll
            for (uint32_t f = 0; f < GV2_FLIGHT; f++) {
                if (k0 + f >= len) break; // (uniform)
#pragma unroll
                for (uint32_t j = 0; j < GV2_COLS; j++) {
                    if (j >= nj) break; // (uniform)
                    const double dse = ds(hd[j], k0 + f);
                    const double u = gv[j] + (double)__uint_as_float(ro[f][j]);
                    const double w = u >= 0.0 ? av[j] : as[j]; // (a NaN u takes the multiplied branch, as gat_leaky_bwd does)
                    const double du = dse * w;
                    dx[j] = dx[j] + du;
                    if constexpr (WITH_P) {
                        const double a = dse * gat_leaky(u, slope);
                        pa[j] = pa[j] + a;
                    }
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < GV2_COLS; j++) {
            const uint32_t i = c0 + lane + 64u * j;
            if (i >= wc) continue;
            if (o64) o64[i] = dx[j];
            if (o32) o32[i] = (float)dx[j];
            if constexpr (WITH_P) p64[i] = pa[j];
        }
    }
}

// The unit of a wave of k_sub_gatv2_bwd and k_sub_gatv2_across, as k_sub_attn cuts it: lane, wave, grp, h0, hc, first, len, wc,
// the rows o32 / o64 / pr of the chunk, ysh, idsh, the places `at` and the staged ids; an empty group has written its +0.0 and
// left, a group past the last or longer than the cap has left.  No lane is past a workgroup barrier: there is none.
#define GV2_UNIT_PROLOGUE                                                                                                             \
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
    const uint32_t wc = hc * d;                                                                                                       \
    float *const o32 = dx32 ? dx32 + (int64_t)grp * ld32 + (uint64_t)h0 * d : nullptr;                                                \
    double *const o64 = dx64 ? dx64 + (int64_t)grp * ld64 + (uint64_t)h0 * d : nullptr;                                               \
    double *const pr = pg ? pg + grp * ((uint64_t)heads * d) + (uint64_t)h0 * d : nullptr;                                            \
    if (count <= 0) {                                                                                                                 \
        for (uint32_t c = lane; c < wc; c += 64u) {                                                                                   \
            if (o64) o64[c] = 0.0;                                                                                                    \
            if (o32) o32[c] = 0.0f;                                                                                                   \
            if (pr) pr[c] = 0.0;                                                                                                      \
        }                                                                                                                             \
        return;                                                                                                                       \
    }                                                                                                                                 \
    const uint32_t len = (uint32_t)count;                                                                                             \
    double *const ysh = sh_y[wave];                                                                                                   \
    int32_t *const idsh = sh_id[wave];                                                                                                \
    uint64_t at[SMAX_PER_LANE];                                                                                                       \
    ssm_places<BYCOL, (int)SMAX_PER_LANE>(pos, first, len, lane, at);                                                                 \
    _Pragma("unroll") for (uint32_t j = 0; j < SMAX_PER_LANE; j++)                                                                    \
        if (lane + 64u * j < len) idsh[lane + 64u * j] = ids[first + lane + 64u * j];

// grid = ceil(ngroups * chunks / SGA_WAVES) workgroups of BLOCK threads, chunks = ceil(heads / SGA_HEADS).  ptr / ids / pos:
// sub_ptr, sub_col and null by row; in_ptr, in_row and in_pos by column.  gs: the operand read at the group (xl by row, xr by
// column), os: the one gathered at the id, both [nc, heads * d]; att: [heads, d]; types = gatv2_types() of the three.  g, v: the
// whole operands, head h their columns [h * dv, (h + 1) * dv); lgv = log2 of the lane group that scores dv columns, gv_types =
// sddmm_types() of the two for ELT_ANY.  y: [heads][edges] in the order of sub_col, f64 when y_f64, else f32.  ds (null: no
// across sum is wanted): [heads][edges] in that order.  dx32 / dx64: the gradient of gs, ngroups x heads * d with their own
// pitches; pg: the P scratch, ngroups x heads * d dense (null: d att is not wanted, WITH_P false); all three null: only ds.
template <int G_ET, int V_ET, bool BYCOL, bool WITH_P>
__global__ void __launch_bounds__(BLOCK) k_sub_gatv2_bwd(const int64_t *__restrict__ ptr, uint32_t ngroups, uint32_t cap, const int32_t *__restrict__ ids,
                                                         const int64_t *__restrict__ pos, uint32_t heads, uint32_t chunks, const void *gs, int64_t ldgs, const void *os,
                                                         int64_t ldos, const void *att, int64_t ldatt, const void *g, int64_t ldg, const void *v, int64_t ldv, uint32_t d,
                                                         uint32_t dv, uint32_t lgv, double slope, uint64_t edges, const void *y, bool y_f64, double *ds, float *dx32,
                                                         int64_t ld32, double *dx64, int64_t ld64, double *pg, uint32_t types, uint32_t gv_types) {
#pragma clang fp contract(off)
    GV2_UNIT_PROLOGUE
    attn_wave_sync();
    // ---- dy, each to its entry's place in the group
    sga_scores<G_ET, V_ET>(idsh, len, hc, g, grp * (uint64_t)ldg, v, ldv, (uint64_t)h0 * dv, dv, lgv, lane, gv_types, ysh);
    attn_wave_sync();
    // ---- D and ds in registers; ds takes the place of dy
    if (len <= 64u) { // (uniform) a lane holds one value of a head, the chunk's heads interleave
        const uint64_t at1[1] = {at[0]};
        if (y_f64) sgb_softmax_bwd<double, 1, SGA_HEADS>(ysh, at1, len, lane, h0, hc, edges, 1.0, (const double *)y, ds);
        else sgb_softmax_bwd<float, 1, SGA_HEADS>(ysh, at1, len, lane, h0, hc, edges, 1.0, (const float *)y, ds);
    } else {
        if (y_f64) sgb_softmax_bwd<double, (int)SMAX_PER_LANE, 1>(ysh, at, len, lane, h0, hc, edges, 1.0, (const double *)y, ds);
        else sgb_softmax_bwd<float, (int)SMAX_PER_LANE, 1>(ysh, at, len, lane, h0, hc, edges, 1.0, (const float *)y, ds);
    }
    if (!o32 && !o64 && !pr) return;
    attn_wave_sync();
    // ---- the gradient row of the group's operand, and P_g
    gatv2_accumulate<WITH_P>(idsh, len, [=](uint32_t h, uint32_t k) { return ysh[h * PROP_SEG + k]; }, gs, grp * (uint64_t)ldgs + (uint64_t)h0 * d, att,
                             (uint64_t)h0 * (uint64_t)ldatt, ldatt, os, ldos, (uint64_t)h0 * d, wc, d, lane, types, slope, o32, o64, pr);
}

// grid and units as k_sub_gatv2_bwd, over the ACROSS side: ptr / ids / pos are sub_ptr, sub_col and null when its groups are
// rows; in_ptr, in_row and in_pos when they are columns.  gs: the operand read at THIS side's group (xr when its groups are
// columns, xl when they are rows), os: the one gathered at the id; types = gatv2_types() in that order.  ds: [heads][edges] in
// the order of sub_col.  dx32 / dx64: the gradient of gs, either may be null.
template <bool BYCOL>
__global__ void __launch_bounds__(BLOCK) k_sub_gatv2_across(const int64_t *__restrict__ ptr, uint32_t ngroups, uint32_t cap, const int32_t *__restrict__ ids,
                                                            const int64_t *__restrict__ pos, uint32_t heads, uint32_t chunks, const void *gs, int64_t ldgs, const void *os,
                                                            int64_t ldos, const void *att, int64_t ldatt, uint32_t d, double slope, uint64_t edges,
                                                            const double *__restrict__ ds, float *dx32, int64_t ld32, double *dx64, int64_t ld64, uint32_t types) {
#pragma clang fp contract(off)
    double *const pg = nullptr;
    GV2_UNIT_PROLOGUE
    for (uint32_t h = 0; h < hc; h++) { // the chunk's ds, each to its entry's place in the group
        const double *const src = ds + (uint64_t)(h0 + h) * edges;
#pragma unroll
        for (uint32_t j = 0; j < SMAX_PER_LANE; j++)
            if (lane + 64u * j < len) ysh[h * PROP_SEG + lane + 64u * j] = src[at[j]];
    }
    attn_wave_sync();
    gatv2_accumulate<false>(idsh, len, [=](uint32_t h, uint32_t k) { return ysh[h * PROP_SEG + k]; }, gs, grp * (uint64_t)ldgs + (uint64_t)h0 * d, att,
                            (uint64_t)h0 * (uint64_t)ldatt, ldatt, os, ldos, (uint64_t)h0 * d, wc, d, lane, types, slope, o32, o64, pr);
}

#undef GV2_UNIT_PROLOGUE

// The longer groups of a side.  grid = ceil(nseg * chunks / SGA_WAVES) workgroups of BLOCK threads: wave u owns segment u / chunks
// of that side's plan and chunk u % chunks.  ids / pos: the side's (pos null when its groups are rows: an entry's place in sub_col
// is its position).  gs, os, att, types: as k_sub_gatv2_across for that side.  ds: [heads][edges] in the order of sub_col.
// part: the partial sums of du, [nseg][heads * d]; part_p: those of a (null: not wanted, WITH_P false).
template <bool WITH_P>
__global__ void __launch_bounds__(BLOCK) k_gatv2_bwd_seg(const PropSeg *__restrict__ segs, uint64_t nseg, const int32_t *__restrict__ ids, const int64_t *__restrict__ pos,
                                                         uint32_t heads, uint32_t chunks, const void *gs, int64_t ldgs, const void *os, int64_t ldos, const void *att,
                                                         int64_t ldatt, uint32_t d, double slope, uint64_t edges, const double *__restrict__ ds, double *part, double *part_p,
                                                         uint32_t types) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t u = (uint64_t)blockIdx.x * SGA_WAVES + wave;
    const uint64_t s = u / chunks;
    if (s >= nseg) return; // (the whole wave)
    const uint32_t h0 = (uint32_t)(u % chunks) * (uint32_t)SGA_HEADS, hc = min((uint32_t)SGA_HEADS, heads - h0);
    const PropSeg sg = segs[s];
    const int64_t *const ps = pos ? pos + sg.first : nullptr;
    const double *const dsc = ds + (uint64_t)h0 * edges;
    const uint64_t row = s * ((uint64_t)heads * d) + (uint64_t)h0 * d;
    gatv2_accumulate<WITH_P>(ids + sg.first, sg.len, [=](uint32_t h, uint32_t k) { return dsc[(uint64_t)h * edges + (ps ? (uint64_t)ps[k] : (uint64_t)(sg.first + k))]; }, gs,
                             (uint64_t)(uint32_t)sg.row * (uint64_t)ldgs + (uint64_t)h0 * d, att, (uint64_t)h0 * (uint64_t)ldatt, ldatt, os, ldos, (uint64_t)h0 * d, hc * d, d, lane,
                             types, slope, nullptr, part + row, WITH_P ? part_p + row : nullptr);
}

// The join of a longer group: the block row of the group's FIRST segment (first == ptr[row]) adds the partial rows of its
// ceil(len / PROP_SEG) segments in order, acc = P_0, acc = acc + P_s, a thread per column.  grid = (ceil(w / BLOCK), min(nseg,
// 65535)).  part_p / pg: the partial sums of a and the P scratch (both null: not wanted).
__global__ void __launch_bounds__(BLOCK) k_gatv2_bwd_join(const PropSeg *__restrict__ segs, uint64_t nseg, const int64_t *__restrict__ ptr, uint32_t w, const double *part,
                                                          const double *part_p, float *dx32, int64_t ld32, double *dx64, int64_t ld64, double *pg) {
#pragma clang fp contract(off)
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= w) return;
    for (uint64_t s = blockIdx.y; s < nseg; s += gridDim.y) {
        const PropSeg sg = segs[s];
        const int64_t lo = ptr[sg.row];
        if (sg.first != lo) continue;
        const uint64_t n = ((uint64_t)(ptr[sg.row + 1] - lo) + PROP_SEG - 1) / PROP_SEG;
        double acc = part[s * w + c], accp = part_p ? part_p[s * w + c] : 0.0;
        for (uint64_t k = 1; k < n; k++) {
            acc = acc + part[(s + k) * w + c];
            if (part_p) accp = accp + part_p[(s + k) * w + c];
        }
        if (dx64) dx64[(int64_t)sg.row * ld64 + c] = acc;
        if (dx32) dx32[(int64_t)sg.row * ld32 + c] = (float)acc;
        if (pg) pg[(uint64_t)(uint32_t)sg.row * w + c] = accp;
    }
}

// One level of the column sum of d att: block row b adds the rows [b * tile, min(rows, (b + 1) * tile)) of src ([rows][w] dense)
// in ascending order from +0.0, a thread per column, to row b of the output -- column c of it at (c / d) * ld + c % d past
// b * stride.  First the tiles of GV2_TILE groups in parallel (d = ld = stride = w: the tile sums, dense), then once over the tile
// sums (tile = rows: d att itself at its pitches).  grid = (ceil(w / BLOCK), min(ceil(rows / tile), 65535)).
__global__ void __launch_bounds__(BLOCK) k_gatv2_datt(const double *__restrict__ src, uint64_t rows, uint64_t tile, uint32_t w, uint32_t d, uint64_t stride, float *o32,
                                                      int64_t ld32, double *o64, int64_t ld64) {
#pragma clang fp contract(off)
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= w) return;
    for (uint64_t b = blockIdx.y; b * tile < rows; b += gridDim.y) {
        const uint64_t r0 = b * tile, r1 = r0 + tile < rows ? r0 + tile : rows;
        double acc = 0.0;
        for (uint64_t r = r0; r < r1; r++) acc = acc + src[r * w + c];
        if (o64) o64[b * stride + (uint64_t)(c / d) * (uint64_t)ld64 + c % d] = acc;
        if (o32) o32[b * stride + (uint64_t)(c / d) * (uint64_t)ld32 + c % d] = (float)acc;
    }
}

} // namespace fora
