/* fora_hip_edge_gatv2_bwd.h -- the entry point of libfora_hip.so for the backward pass of GATv2 attention over the edges of the
 * held subgraph, all heads in ONE call, beside those of fora_hip.h, fora_hip_ext.h, fora_hip_gnn.h, fora_hip_edge.h,
 * fora_hip_edge_softmax.h, fora_hip_edge_attention.h, fora_hip_edge_attention_bwd.h, fora_hip_edge_gat.h, fora_hip_pool.h and
 * fora_hip_edge_gatv2.h: the same library, the same fora_ctx, the same return codes.  Plain C99; three gradients leave through the
 * fora_attn_grads of fora_hip.h, the fourth and the statistics through out-pointers, so this header declares no struct of its own.
 *
 * EDGE GATV2, BACKWARD (fora_hip_subgraph_gatv2_bwd): the gradients of EDGE GATV2 (fora_hip_edge_gatv2.h) with respect to xl, xr,
 * att and v for all heads in one call, as EDGE GAT, BACKWARD (fora_hip_edge_gat.h) is for the additive score.
 *   - inputs: the forward call's xl, xr, att and v with their four independently chosen element types and their pitches, d, dv,
 *     heads, slope and flags; g = dL/dout, [nc, heads * dv], any element type of PROPAGATE, at pitch ldg >= heads * dv; y, the
 *     probabilities the forward call returned, [heads][edges], y_type FORA_PROP_F32 or FORA_PROP_F64, ycap the elements it holds,
 *     at least heads * edges.  Host memory or the ctx's GPU, read in place.
 *   - outputs: the fora_attn_grads of fora_hip.h -- dq32 / dq64 at pitch lddq carry d xl, dk32 / dk64 at lddk carry d xr, both
 *     [nc, heads * d]; dv32 / dv64 at lddv carry dv, [nc, heads * dv]; datt32 / datt64 at pitch lddatt >= d carry d att,
 *     [heads, d]; host or device memory.  A gradient with both pointers NULL is absent and costs nothing; with d xl, d xr and d att
 *     all absent dy, ds and du are never computed and xl, xr, att and v are not read.
 *   - the bits: per head h, with ALONG the forward call's grouping and ACROSS the opposite one, everything chained through f64
 *     and nothing rounded to f32 in between:
 *       dy, ds, dv: exactly as EDGE GAT, BACKWARD words them -- dy = EDGE SCORES in f64 of (g, v) with flags = 0 and of (v, g)
 *            with FORA_SUB_BY_COL on the dv-wide slice; ds = EDGE SOFTMAX backward of (y[h], dy), the same flags, scale = 1.0;
 *            dv = the across SUBGRAPH PRODUCT of the g slice with y[h], in the caller's type, as values;
 *       u_e[c]  = (double)xl[row(e), h*d + c] + (double)xr[sub_col[e], h*d + c], computed again as EDGE GATV2 has it -- one f64
 *                 addition;
 *       t_e[c]  = (u_e[c] >= 0.0) ? u_e[c] : u_e[c] * slope;
 *       w_e[c]  = (u_e[c] >= 0.0) ? (double)att[h, c] : (double)att[h, c] * slope -- one f64 multiplication; a NaN u takes the
 *                 multiplied branch;
 *       du_e[c] = ds_e * w_e[c] -- one f64 multiplication, which rounds;
 *       a_e[c]  = ds_e * t_e[c] -- one f64 multiplication, which rounds;
 *       the gradient of the operand read at the GROUP's node -- xl with flags = 0, xr with FORA_SUB_BY_COL -- is, for each output
 *            row and column, the sum of du_e[c] over the group's entries in the SUBGRAPH PRODUCT's order of additions
 *            (fora_hip_gnn.h): the terms are added in entry order from +0.0 inside segments of FORA_PROP_SEG = 256 entries, and
 *            the segments' sums are added in order, acc = P_0, acc = acc + P_s;
 *       the gradient of the operand at the OTHER end is the same sum over the across group's entries -- in ascending e when the
 *            across groups are columns, in row order when they are rows -- with the same segment rule;
 *       d att[h, c]: P_g[h, c] is the ALONG group g's sum of a_e[c] in that same order (an empty group: +0.0); T_b is the sum of
 *            P_g over the FORA_GATV2_DATT_TILE = 256 consecutive groups g = 256 b .. 256 b + 255 of tile b, ascending from +0.0;
 *            d att is the sum of the T_b, ascending from +0.0.
 *     The f32 outputs are the f64 ones rounded once.  A node with no edge on the side that sums gets +0.0.  No bit depends on the
 *     launch shape, on any option ("attn_short" among them, which bounds the groups of BOTH sides that one wave handles, as in
 *     EDGE ATTENTION, BACKWARD), or on host versus device pointers; for d xl, d xr and dv none depends on heads being one call or
 *     `heads` calls with heads = 1 on column slices (d att row h is then the one-head call's as well: its sum runs over groups,
 *     not heads).
 *   - non-finite values follow IEEE as in EDGE GAT, BACKWARD: nothing is checked, written in place of a result, or counted.
 *   - the transposition is built by the first call that needs it: every call but one with flags = 0 that wants neither d xr nor
 *     dv, or one over a subgraph of 0 edges.
 *   - info_out (NULL or six int64: edges, the along side's short and longer groups, the across side's, built), ms_out (NULL or
 *     two doubles: the one-wave kernels, the longer groups' kernels), lifetime, "only reads the held result": as EDGE GAT,
 *     BACKWARD.  There is no new option and no new state word.
 *   - errors: as EDGE GATV2 for xl, xr, att, v, d, dv, heads, slope and flags, and as EDGE GAT, BACKWARD for g, y, y_type, ycap
 *     and grads: a pitch of a wanted gradient below its width (heads * d for d xl and d xr, heads * dv for dv, lddatt < d for
 *     d att), y_type neither f32 nor f64, grads NULL with no d att or all four gradients absent, ycap < heads * edges, a NULL xl,
 *     xr, att, v, g or y when there are edges: FORA_E_ARG, nothing written.  No device memory: FORA_E_NOMEM, nothing changed.
 *     nc = 0: FORA_OK, nothing launched.  A subgraph of 0 edges: every wanted gradient is +0.0.
 */
#ifndef FORA_HIP_EDGE_GATV2_BWD_H
#define FORA_HIP_EDGE_GATV2_BWD_H
#include "fora_hip_edge_gatv2.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FORA_GATV2_DATT_TILE 256

/* ---- the gradients of GATv2 attention over the held subgraph (the EDGE GATV2, BACKWARD contract above) */
int fora_hip_subgraph_gatv2_bwd(fora_ctx *ctx,
        const void *xl /*[nc, heads*d]*/, int xl_type, int64_t ldxl, const void *xr /*[nc, heads*d]*/, int xr_type, int64_t ldxr,
        const void *att /*[heads, d]*/, int att_type, int64_t ldatt, const void *v /*[nc, heads*dv]*/, int v_type, int64_t ldv,
        const void *g /*[nc, heads*dv]*/, int g_type, int64_t ldg, const void *y /*[heads][edges]*/, int y_type, uint64_t ycap,
        int d, int dv, int heads, double slope, int flags, const fora_attn_grads *grads,
        float *datt32 /*or NULL*/, double *datt64 /*or NULL*/, int64_t lddatt, int64_t *info_out /*6 or NULL*/, double *ms_out /*2 or NULL*/);

#ifdef __cplusplus
}
#endif
#endif
