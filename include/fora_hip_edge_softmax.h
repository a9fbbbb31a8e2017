/* fora_hip_edge_softmax.h -- the entry points of libfora_hip.so for the softmax over the edges of the held subgraph, beside those
 * of fora_hip.h, fora_hip_ext.h, fora_hip_gnn.h and fora_hip_edge.h: the same library, the same fora_ctx, the same return codes.
 * Plain C99; statistics leave through out-pointers, so this header declares no struct of its own.
 *
 * EDGE SOFTMAX (fora_hip_subgraph_softmax, fora_hip_subgraph_softmax_bwd): the step between EDGE SCORES (fora_hip_edge.h) and
 * SUBGRAPH PRODUCTS with values (fora_hip_gnn.h) of a GAT or graph-transformer layer over the held subgraph A_S of
 * fora_hip_sparse_subgraph -- for every head, the softmax over each node's edges, and its gradient.
 *   - layout: scores, y, g and the outputs are [heads][edges] without a pitch, the edges in the order of sub_col: exactly what
 *     fora_hip_subgraph_sddmm writes, and one head's outputs are what `values` of SUBGRAPH PRODUCTS takes as they are.  s_type,
 *     y_type and g_type are each FORA_PROP_F32 or FORA_PROP_F64, each operand on its own.  Operands and outputs lie in host
 *     memory or on the ctx's GPU and are read and written in place.  out32 (float) and out64 (double), at least one; ocap: the
 *     elements each can take, at least heads * edges.  out32 is out64 rounded once.
 *   - groups: with flags = 0 a group is a ROW j of the subgraph: the places sub_ptr[j] .. sub_ptr[j + 1] of sub_col, in that
 *     order -- the softmax over the out-edges of cols[j], which fora_hip_subgraph_propagate aggregates over.  With
 *     FORA_SUB_BY_COL a group is a COLUMN v: the places in_pos[in_ptr[v] .. in_ptr[v + 1]) of the subgraph's transposition, in
 *     that order -- the softmax over the in-edges of cols[v], which fora_hip_subgraph_propagate_t aggregates over.  The
 *     transposition is the one fora_hip_subgraph_transpose_fetch returns, built by the first call that needs it and kept with
 *     the subgraph.  The outputs are in edge order whichever the grouping.  An empty group writes nothing.
 *   - the bits: per head and per group, the ROW SOFTMAX contract of fora_hip.h applied unchanged to the group's sequence of
 *     values: x = (double)score * scale; m = the largest x; p = exp_def(x - m); S = the sum of p -- inside a segment of
 *     FORA_PROP_SEG = 256 entries the 64 running sums q_l over the positions j == l (mod 64) in ascending j from +0.0, the
 *     tree q_l = q_l + q_{l+o} for o = 32 .. 1, the segments' sums added in order --; y = p / S.  Backward: t = (double)y *
 *     (double)g, D = the sum of t in the same order, dx = ((g - D) * y) * scale, y the forward output and scale its scale.
 *     No bit depends on the launch shape, on heads being one call or `heads` calls with heads = 1 on the [edges] slices, or on
 *     any option.  The option "softmax_short" of ROW SOFTMAX is reused with its meaning and clamp (0 .. 256): a group of at
 *     most that many entries is one wave's; a longer one goes segment by segment; 0: every group does.
 *   - NaN: a (group, head) with a NaN, with +inf, or of -inf only is written as the quiet NaN 0x7FF8000000000000 (out32:
 *     rounded from it) and counted in info_out[2]; its neighbours are unaffected.  scale must be finite.
 *   - info_out (NULL or four int64): the edges; the groups longer than "softmax_short"; the NaN (group, head) pairs (0
 *     backward); 1 if this call built the transposition.  ms_out (NULL or two doubles): device time of the short and of the
 *     long path -- each 0 with the option "profile" off.
 *   - lifetime: as EDGE SCORES -- the calls work on the held subgraph and take no row_ptr; no subgraph held: FORA_E_ARG.  They
 *     only read the held result: the subgraph's arrays, "sparse_generation", the held ids and words, the contents of both
 *     transpositions, the store, the options and fora_timing are untouched.  The segment list of the longer groups is made
 *     once per held subgraph, grouping and value of "softmax_short", kept with the subgraph and ends where it ends.
 *   - errors: a NULL ctx is answered without touching the GPU (FORA_E_ARG).  heads < 1, a type that is neither f32 nor f64, an
 *     unknown flag bit (FORA_SUB_MEAN among them), a scale that is not finite, both outputs NULL, ocap < heads * edges, a
 *     NULL operand when there are edges, memory of another GPU: FORA_E_ARG, nothing written.  No device memory:
 *     FORA_E_NOMEM, nothing changed.  nc = 0 or a subgraph of 0 edges: FORA_OK, nothing launched or written.  The ctx's
 *     stream is idle when the calls return.
 */
#ifndef FORA_HIP_EDGE_SOFTMAX_H
#define FORA_HIP_EDGE_SOFTMAX_H
#include "fora_hip_edge.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FORA_SUB_BY_COL 2 /* flags: a group is a column of the subgraph (its in-edges), not a row; a bit FORA_SUB_MEAN does not use */

/* ---- softmax over each node's edges of the held subgraph (the EDGE SOFTMAX contract above) */
int fora_hip_subgraph_softmax(fora_ctx *ctx, const void *scores /*[heads][edges]*/, int s_type, int heads, double scale, int flags,
                              float *out32 /*or NULL*/, double *out64 /*or NULL*/, uint64_t ocap,
                              int64_t *info_out /*4 or NULL*/, double *ms_out /*2 or NULL*/);
int fora_hip_subgraph_softmax_bwd(fora_ctx *ctx, const void *y /*[heads][edges]*/, int y_type, const void *g /*[heads][edges]*/, int g_type,
                                  int heads, double scale, int flags, float *out32 /*or NULL*/, double *out64 /*or NULL*/, uint64_t ocap,
                                  int64_t *info_out /*4 or NULL*/, double *ms_out /*2 or NULL*/);

#ifdef __cplusplus
}
#endif
#endif
