/* fora_hip_edge_gat.h -- the entry points of libfora_hip.so for graph attention (GAT) over the edges of the held subgraph, forward
 * and backward in ONE call each, beside those of fora_hip.h, fora_hip_ext.h, fora_hip_gnn.h, fora_hip_edge.h,
 * fora_hip_edge_softmax.h, fora_hip_edge_attention.h and fora_hip_edge_attention_bwd.h: the same library, the same fora_ctx, the
 * same return codes.  Plain C99; the gradients leave through the fora_attn_grads of fora_hip.h and statistics through
 * out-pointers, so this header declares no struct of its own.
 *
 * EDGE GAT (fora_hip_subgraph_gat): EDGE ATTENTION (fora_hip_edge_attention.h) with the ADDITIVE score of a graph attention
 * network in place of the dot product: LeakyReLU(el[row] + er[col]), el and er one scalar per node and head -- what
 * (feat * attn_l).sum(-1) and (feat * attn_r).sum(-1) give in a GATConv layer.
 *   - operands: el and er are [nc, heads] at pitches ldel, lder >= heads; v is [nc, heads * dv] at pitch ldv >= heads * dv, head
 *     h its columns [h*dv, (h+1)*dv).  el_type, er_type and v_type are each an element type of PROPAGATE (FORA_PROP_F32, _BF16,
 *     _F16, _E4M3, _E5M2), chosen independently; each operand lives in host memory or on the ctx's GPU and is read in place; a
 *     column slice is an operand.  slope, the LeakyReLU's, is a finite double.  flags: 0 or FORA_SUB_BY_COL.
 *   - outputs, groups: as EDGE ATTENTION -- out32 / out64, at least one, [nc, heads * dv] at pitch ldo; y32 / y64, both optional,
 *     [heads][edges] in the order of sub_col, ycap the elements each takes.  With flags = 0 node j attends over its out-edges
 *     (row j of sub_ptr) and out[j] sums v[sub_col[e]]; with FORA_SUB_BY_COL node u attends over its in-edges (the positions
 *     [in_ptr[u], in_ptr[u + 1]) of the transposition) and out[u] sums v[in_row[p]] in ascending e.
 *   - the bits: per head h, a composition of contracts that exist, chained through f64:
 *       z_e = (double)el[row(e), h] + (double)er[sub_col[e], h] -- one f64 addition; el is read at the edge's ROW and er at its
 *             COLUMN under both groupings: the grouping decides only what is normalised together and which end aggregates;
 *       s_e = (z_e >= 0.0) ? z_e : z_e * slope -- one f64 multiplication; a NaN z stays NaN, -0.0 stays -0.0;
 *       y   = EDGE SOFTMAX (fora_hip_edge_softmax.h) of s: FORA_PROP_F64 in, out64, the same flags, scale = 1.0;
 *       out = the SUBGRAPH PRODUCT (fora_hip_gnn.h) of the head's slice of v with the f64 y[h] as values:
 *             fora_hip_subgraph_propagate with flags = 0, fora_hip_subgraph_propagate_t with FORA_SUB_BY_COL.
 *     Nothing is rounded to f32 in between; out32 = (float)out64, y32 = (float)y64.  No bit depends on the launch shape, on heads
 *     being one call or `heads` calls with heads = 1 on column slices, on host versus device pointers, or on any option.  The
 *     option "attn_short" keeps its meaning and clamp (0 .. 256): a non-empty group of at most that many edges is scored,
 *     normalised and multiplied by one wave; a longer one goes head by head through the kernels of the steps inside the same
 *     call, steered by "softmax_short" and "prop_segs" as those steps are; 0: every group does.
 *   - NaN: EDGE ATTENTION's rule.  A (group, head) with a NaN score, with a maximum of +inf, or of -inf only is written, not
 *     computed: the quiet NaN 0x7FF8000000000000 to its y and to its dv outputs (out32, y32: rounded from it), counted per pair in
 *     info_out[3]; its neighbours are unaffected.  An empty group writes +0.0 to its heads * dv outputs and nothing to y.
 *   - info_out (NULL or five int64), ms_out (NULL or two doubles), lifetime, the plans kept with the subgraph, "only reads the
 *     held result": as EDGE ATTENTION.
 *   - errors: a NULL ctx is answered without touching the GPU (FORA_E_ARG).  No subgraph held, dv or heads < 1, heads * dv >
 *     65536, a pitch below its matrix' width, a type code that is no type, an unknown flag bit (FORA_SUB_MEAN among them), a
 *     slope that is not finite, both out pointers NULL, ycap < heads * edges with a y pointer that is not NULL, a NULL operand when
 *     there are edges, memory of another GPU: FORA_E_ARG, nothing written.  No device memory: FORA_E_NOMEM, nothing changed.
 *     nc = 0: FORA_OK, nothing launched.  A subgraph of 0 edges: every output row is +0.0.  The ctx's stream is idle when the
 *     call returns.
 *
 * EDGE GAT, BACKWARD (fora_hip_subgraph_gat_bwd): the gradients of EDGE GAT with respect to el, er and v for all heads in one
 * call, as EDGE ATTENTION, BACKWARD (fora_hip_edge_attention_bwd.h) is for the dot-product score.
 *   - inputs: the forward call's el, er, v with their types and pitches, dv, heads, slope and flags; g = dL/dout, [nc, heads * dv],
 *     any element type of PROPAGATE, at pitch ldg >= heads * dv; y, the probabilities the forward call returned, [heads][edges],
 *     y_type FORA_PROP_F32 or FORA_PROP_F64, ycap the elements it holds, at least heads * edges.
 *   - the gradients: per head h, with ALONG the forward call's grouping and ACROSS the opposite one:
 *       dy = EDGE SCORES (fora_hip_edge.h) in f64 of (g, v) with flags = 0 and of (v, g) with FORA_SUB_BY_COL, on the dv-wide
 *            slice -- g is the operand read at the group;
 *       ds = EDGE SOFTMAX backward of (y[h], dy) with the same flags and scale = 1.0, the output f64;
 *       dz_e = (z_e >= 0.0) ? ds_e : ds_e * slope, z computed again from el and er as above;
 *       the gradient of the operand read at the GROUP's node -- el with flags = 0, er with FORA_SUB_BY_COL -- is the along
 *            SUBGRAPH PRODUCT of a column of ones, [nc, 1] f32, with the f64 dz[h] as values: the contract's ordered sum of dz,
 *            since dz * 1.0 is exact;
 *       the gradient of the operand at the OTHER end is the across product of the ones column with dz[h];
 *       dv = the across product of the g slice with y[h], in the caller's type, as values.
 *   - outputs: the fora_attn_grads of fora_hip.h -- dq32 / dq64 at pitch lddq carry d el, dk32 / dk64 at lddk carry d er, both
 *     [nc, heads]; dv32 / dv64 at lddv carry dv, [nc, heads * dv]; host or device memory.  A gradient with both pointers NULL is
 *     absent and costs nothing; with d el and d er both absent dy, ds and dz are never computed and v, el and er are not read.
 *     A node with no edge on the side that sums gets +0.0.
 *   - non-finite values follow IEEE as in EDGE SOFTMAX backward: nothing is checked, written in place of a result, or counted.
 *     Where a NaN is involved the chained calls agree in NaN-ness only.
 *   - the transposition is built by the first call that needs it: every call but one with flags = 0 that wants d el alone, or one
 *     over a subgraph of 0 edges.
 *   - info_out (NULL or six int64), ms_out (NULL or two doubles), lifetime, "attn_short" bounding the groups of BOTH sides that
 *     one wave handles: as EDGE ATTENTION, BACKWARD.
 *   - errors: as EDGE GAT, and as EDGE ATTENTION, BACKWARD for g, y, y_type, ycap and grads: a pitch of a wanted gradient below
 *     its width (heads for d el and d er), y_type neither f32 nor f64, grads NULL or all three gradients absent, ycap < heads *
 *     edges, a NULL el, er, v, g or y when there are edges: FORA_E_ARG, nothing written.
 */
#ifndef FORA_HIP_EDGE_GAT_H
#define FORA_HIP_EDGE_GAT_H
#include "fora_hip_edge_attention_bwd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- graph attention over each node's edges of the held subgraph (the EDGE GAT contract above) */
int fora_hip_subgraph_gat(fora_ctx *ctx,
        const void *el /*[nc, heads]*/, int el_type, int64_t ldel, const void *er /*[nc, heads]*/, int er_type, int64_t lder,
        const void *v /*[nc, heads*dv]*/, int v_type, int64_t ldv, int dv, int heads, double slope, int flags,
        float *out32 /*or NULL*/, double *out64 /*or NULL*/, int64_t ldo,
        float *y32 /*or NULL*/, double *y64 /*or NULL*/, uint64_t ycap,
        int64_t *info_out /*5 or NULL*/, double *ms_out /*2 or NULL*/);

/* ---- its gradients (the EDGE GAT, BACKWARD contract above) */
int fora_hip_subgraph_gat_bwd(fora_ctx *ctx,
        const void *el /*[nc, heads]*/, int el_type, int64_t ldel, const void *er /*[nc, heads]*/, int er_type, int64_t lder,
        const void *v /*[nc, heads*dv]*/, int v_type, int64_t ldv, const void *g /*[nc, heads*dv]*/, int g_type, int64_t ldg,
        const void *y /*[heads][edges]*/, int y_type, uint64_t ycap, int dv, int heads, double slope, int flags,
        const fora_attn_grads *grads, int64_t *info_out /*6 or NULL*/, double *ms_out /*2 or NULL*/);

#ifdef __cplusplus
}
#endif
#endif
