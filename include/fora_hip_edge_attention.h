/* fora_hip_edge_attention.h -- the entry point of libfora_hip.so for attention over the edges of the held subgraph in ONE call,
 * beside those of fora_hip.h, fora_hip_ext.h, fora_hip_gnn.h, fora_hip_edge.h and fora_hip_edge_softmax.h: the same library, the
 * same fora_ctx, the same return codes.  Plain C99; statistics leave through out-pointers, so this header declares no struct of
 * its own.
 *
 * EDGE ATTENTION (fora_hip_subgraph_attention): a GAT or graph-transformer layer over the held subgraph A_S of
 * fora_hip_sparse_subgraph -- EDGE SCORES (fora_hip_edge.h), EDGE SOFTMAX (fora_hip_edge_softmax.h) and SUBGRAPH PRODUCTS with
 * values (fora_hip_gnn.h) for all heads, with nothing written between the steps.
 *   - operands: q and k are [nc, heads * d], v is [nc, heads * dv]; head h reads the columns [h*d, (h+1)*d) of q and k and
 *     [h*dv, (h+1)*dv) of v.  q_type, k_type and v_type are each an element type of PROPAGATE (FORA_PROP_F32, _BF16, _F16, _E4M3,
 *     _E5M2), chosen independently; each matrix lives in host memory or on the ctx's GPU and is read in place at any pitch ldq,
 *     ldk >= heads * d, ldv >= heads * dv.
 *   - outputs: out32 (float) and out64 (double), at least one, each [nc, heads * dv] at pitch ldo >= heads * dv; y32 and y64, the
 *     probabilities, both optional, each [heads][edges] without a pitch in the order of sub_col -- the layout of EDGE SCORES and
 *     EDGE SOFTMAX; ycap: the elements each y can take, at least heads * edges.  All in host or device memory.
 *   - groups: with flags = 0 node j attends over its OUT-edges: the group is row j of sub_ptr, score_e = <q[j], k[sub_col[e]]> on
 *     the head's slice, out[j] = the sum over the row's edges e, in the order of sub_col, of y_e * v[sub_col[e]].  With
 *     FORA_SUB_BY_COL node u attends over its IN-edges: the group is the positions p of [in_ptr[u], in_ptr[u + 1]) of the
 *     transposition (fora_hip_subgraph_transpose_fetch; built by the first call that needs it and kept with the subgraph), the
 *     edge is e = in_pos[p] and its row in_row[p]; score_e = <k[in_row[p]], q[u]> -- EDGE SCORES with a = k, b = q -- and out[u] =
 *     the sum in ascending e of y_e * v[in_row[p]] -- fora_hip_subgraph_propagate_t with values.
 *   - the bits: per head, every output bit is the composition, on the head's column slices, of EDGE SCORES (out64), EDGE SOFTMAX
 *     (FORA_PROP_F64 in, out64, the same flags and scale) and SUBGRAPH PRODUCTS with those f64 values; nothing is rounded to f32 in
 *     between.  out32 = (float)out64, y32 = (float)y64.  No bit depends on the launch shape, on heads being one call or `heads`
 *     calls with heads = 1 on column slices, on host versus device pointers, or on any option.  The option "attn_short" of
 *     ATTENTION is reused with its meaning and clamp (0 .. 256): a non-empty group of at most that many edges is scored, normalised
 *     and multiplied by one wave; a longer one goes through the kernels of the three steps inside the same call; 0: every group
 *     does.  "softmax_short" and "prop_segs" steer the longer groups as they steer those steps.
 *   - NaN: a (group, head) with a NaN score, with a maximum of +inf, or of -inf only follows ROW SOFTMAX's rule and is written,
 *     not computed: the quiet NaN 0x7FF8000000000000 to its y and to its dv outputs (out32, y32: rounded from it), counted per
 *     (group, head) pair in info_out[3]; its neighbours are unaffected.  On such a group the chained calls agree in NaN-ness only,
 *     as the ATTENTION contract of fora_hip.h says.  An empty group writes +0.0 to its heads * dv outputs and nothing to y.
 *     scale must be finite.
 *   - info_out (NULL or five int64): the edges; the non-empty groups of at most "attn_short" edges; the longer groups; the NaN
 *     (group, head) pairs; 1 if this call built the transposition.  ms_out (NULL or two doubles): device time of the fused kernel
 *     and of the longer groups' path -- each 0 with the option "profile" off.
 *   - lifetime: as EDGE SOFTMAX -- the call works on the held subgraph and takes no row_ptr; no subgraph held: FORA_E_ARG.  It
 *     only reads the held result: the subgraph's arrays, "sparse_generation", the held ids and words, the contents of both
 *     transpositions, the store, the options and fora_timing are untouched.  The plan and the segment lists of the longer groups
 *     are made once per held subgraph, grouping and values of the options above, kept with the subgraph and end where it ends.
 *   - errors: a NULL ctx is answered without touching the GPU (FORA_E_ARG).  d, dv or heads < 1, heads * d or heads * dv >
 *     65536, a pitch below its matrix' width, a type code that is no type, an unknown flag bit (FORA_SUB_MEAN among them), a
 *     scale that is not finite, both out pointers NULL, ycap < heads * edges with a y pointer that is not NULL, a NULL operand when
 *     there are edges, memory of another GPU: FORA_E_ARG, nothing written.  No device memory: FORA_E_NOMEM, nothing changed.
 *     nc = 0: FORA_OK, nothing launched.  A subgraph of 0 edges: every output row is +0.0.  The ctx's stream is idle when the
 *     call returns.
 */
#ifndef FORA_HIP_EDGE_ATTENTION_H
#define FORA_HIP_EDGE_ATTENTION_H
#include "fora_hip_edge_softmax.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- attention over each node's edges of the held subgraph (the EDGE ATTENTION contract above) */
int fora_hip_subgraph_attention(fora_ctx *ctx,
        const void *q /*[nc, heads*d]*/, int q_type, int64_t ldq, const void *k /*[nc, heads*d]*/, int k_type, int64_t ldk,
        const void *v /*[nc, heads*dv]*/, int v_type, int64_t ldv, int d, int dv, int heads, double scale, int flags,
        float *out32 /*or NULL*/, double *out64 /*or NULL*/, int64_t ldo,
        float *y32 /*or NULL*/, double *y64 /*or NULL*/, uint64_t ycap,
        int64_t *info_out /*5 or NULL*/, double *ms_out /*2 or NULL*/);

#ifdef __cplusplus
}
#endif
#endif
