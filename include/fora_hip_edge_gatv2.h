/* fora_hip_edge_gatv2.h -- the entry point of libfora_hip.so for GATv2 attention over the edges of the held subgraph, the forward
 * pass in ONE call, beside those of fora_hip.h, fora_hip_ext.h, fora_hip_gnn.h, fora_hip_edge.h, fora_hip_edge_softmax.h,
 * fora_hip_edge_attention.h, fora_hip_edge_attention_bwd.h, fora_hip_edge_gat.h and fora_hip_pool.h: the same library, the same
 * fora_ctx, the same return codes.  Plain C99; statistics leave through out-pointers, so this header declares no struct of its own.
 *
 * EDGE GATV2 (fora_hip_subgraph_gatv2): EDGE GAT (fora_hip_edge_gat.h) with the score of GATv2 ("How attentive are graph attention
 * networks?"; GATv2Conv) -- the non-linearity INSIDE the sum, so that the score does not factor into a scalar per end:
 *     s_e[h] = sum over c < d of att[h, c] * LeakyReLU(xl[row(e), h*d + c] + xr[sub_col[e], h*d + c]).
 *   - operands: xl and xr are [nc, heads * d] at pitches ldxl, ldxr >= heads * d, head h their columns [h*d, (h+1)*d); they may be
 *     the same pointer (shared weights).  att is [heads, d] at pitch ldatt >= d.  v is [nc, heads * dv] at pitch ldv >= heads * dv.
 *     xl_type, xr_type, att_type and v_type are each an element type of PROPAGATE (FORA_PROP_F32, _BF16, _F16, _E4M3, _E5M2),
 *     chosen independently; each operand lives in host memory or on the ctx's GPU and is read in place at its pitch; a column
 *     slice is an operand.  slope, the LeakyReLU's, is a finite double.  flags: 0 or FORA_SUB_BY_COL.
 *   - outputs, groups: as EDGE GAT -- out32 / out64, at least one, [nc, heads * dv] at pitch ldo; y32 / y64, both optional,
 *     [heads][edges] in the order of sub_col, ycap the elements each takes.  With flags = 0 node j attends over its out-edges
 *     (row j of sub_ptr) and out[j] sums v[sub_col[e]]; with FORA_SUB_BY_COL node u attends over its in-edges (the positions
 *     [in_ptr[u], in_ptr[u + 1]) of the transposition) and out[u] sums v[in_row[p]] in ascending e.
 *   - the bits: per head h, chained through f64 with nothing rounded to f32 in between:
 *       u_e[c]    = (double)xl[row(e), h*d + c] + (double)xr[sub_col[e], h*d + c] -- one f64 addition; xl is read at the edge's
 *                   ROW and xr at its COLUMN under both groupings: the grouping decides only what is normalised together and
 *                   which end aggregates;
 *       t_e[c]    = (u_e[c] >= 0.0) ? u_e[c] : u_e[c] * slope -- one f64 multiplication; a NaN stays NaN, -0.0 stays -0.0;
 *       term_e[c] = (double)att[h, c] * t_e[c] -- one f64 multiplication, which ROUNDS (unlike the exact products of EDGE SCORES);
 *       s_e       = the sum of term_e[0 .. d) in the order of additions of SCORES (fora_hip.h): running sums q_l over
 *                   c == l (mod 64) in ascending c from +0.0, then the tree o = 32 .. 1, q_l = q_l + q_{l+o} for l < o, s_e = q_0;
 *       y         = EDGE SOFTMAX (fora_hip_edge_softmax.h) of s: FORA_PROP_F64 in, out64, the same flags, scale = 1.0;
 *       out       = the SUBGRAPH PRODUCT (fora_hip_gnn.h) of the head's slice of v with the f64 y[h] as values:
 *                   fora_hip_subgraph_propagate with flags = 0, fora_hip_subgraph_propagate_t with FORA_SUB_BY_COL.
 *     out32 = (float)out64, y32 = (float)y64.  No bit depends on the launch shape, on any option, on host versus device pointers,
 *     or on heads being one call or `heads` calls with heads = 1 on column slices (with row h of att as a one-row operand).  The
 *     option "attn_short" keeps its meaning and clamp (0 .. 256): a non-empty group of at most that many edges is scored,
 *     normalised and multiplied by one wave; a longer one goes head by head through the kernels of the steps inside the same
 *     call, steered by "softmax_short" and "prop_segs" as those steps are; 0: every group does.
 *   - NaN: EDGE GAT's rule.  A (group, head) with a NaN score, with a maximum of +inf, or of -inf only is written, not computed:
 *     the quiet NaN 0x7FF8000000000000 to its y and to its dv outputs (out32, y32: rounded from it), counted per pair in
 *     info_out[3]; its neighbours are unaffected.  An empty group writes +0.0 to its heads * dv outputs and nothing to y.
 *   - info_out (NULL or five int64), ms_out (NULL or two doubles), lifetime, the plans kept with the subgraph, "only reads the
 *     held result": as EDGE GAT.  There is no new option and no new state word.
 *   - errors: a NULL ctx is answered without touching the GPU (FORA_E_ARG).  No subgraph held, d, dv or heads < 1, heads * d or
 *     heads * dv > 65536, a pitch below its matrix' width (ldxl or ldxr below heads * d, ldatt below d, ldv or ldo below
 *     heads * dv), a type code that is no type, an unknown flag bit (FORA_SUB_MEAN among them), a slope that is not finite, both
 *     out pointers NULL, ycap < heads * edges with a y pointer that is not NULL, a NULL xl, xr, att or v when there are edges,
 *     memory of another GPU: FORA_E_ARG, nothing written.  No device memory: FORA_E_NOMEM, nothing changed.  nc = 0: FORA_OK,
 *     nothing launched.  A subgraph of 0 edges: every output row is +0.0.  The ctx's stream is idle when the call returns.
 *   - the gradients are not part of this header: a layer's backward pass composes EDGE SCORES, EDGE SOFTMAX backward and the
 *     SUBGRAPH PRODUCT with the framework's own operations (fora_amd.torch_ops.subgraph_gatv2).
 */
#ifndef FORA_HIP_EDGE_GATV2_H
#define FORA_HIP_EDGE_GATV2_H
#include "fora_hip_edge_gat.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- GATv2 attention over each node's edges of the held subgraph (the EDGE GATV2 contract above) */
int fora_hip_subgraph_gatv2(fora_ctx *ctx,
        const void *xl /*[nc, heads*d]*/, int xl_type, int64_t ldxl, const void *xr /*[nc, heads*d]*/, int xr_type, int64_t ldxr,
        const void *att /*[heads, d]*/, int att_type, int64_t ldatt, const void *v /*[nc, heads*dv]*/, int v_type, int64_t ldv,
        int d, int dv, int heads, double slope, int flags,
        float *out32 /*or NULL*/, double *out64 /*or NULL*/, int64_t ldo,
        float *y32 /*or NULL*/, double *y64 /*or NULL*/, uint64_t ycap,
        int64_t *info_out /*5 or NULL*/, double *ms_out /*2 or NULL*/);

#ifdef __cplusplus
}
#endif
#endif
