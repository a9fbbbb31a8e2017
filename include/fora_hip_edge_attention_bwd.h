/* fora_hip_edge_attention_bwd.h -- the entry point of libfora_hip.so for the gradients of attention over the edges of the held
 * subgraph in ONE call, beside those of fora_hip.h, fora_hip_ext.h, fora_hip_gnn.h, fora_hip_edge.h, fora_hip_edge_softmax.h and
 * fora_hip_edge_attention.h: the same library, the same fora_ctx, the same return codes.  Plain C99; the outputs are the
 * fora_attn_grads of fora_hip.h, statistics leave through out-pointers, so this header declares no struct of its own.
 *
 * EDGE ATTENTION, BACKWARD (fora_hip_subgraph_attention_bwd): the gradients of EDGE ATTENTION (fora_hip_subgraph_attention) with
 * respect to q, k and v, for all heads in one call -- as ATTENTION, BACKWARD of fora_hip.h is for the held rows, a composition of
 * contracts that exist, with nothing written or rounded between the steps.
 *   - inputs: the forward call's q, k, v with their types and pitches, d, dv, heads, scale and flags (0 or FORA_SUB_BY_COL);
 *     g = dL/dout, [nc, heads * dv], any element type of PROPAGATE, at pitch ldg >= heads * dv; y, the probabilities the forward
 *     call returned, [heads][edges] in the order of sub_col, y_type FORA_PROP_F32 or FORA_PROP_F64, ycap the elements it holds,
 *     at least heads * edges.  Each lives in host memory or on the ctx's GPU and is read in place; a column slice is an operand.
 *   - the gradients: per head h, on the head's column slices, with ALONG the forward call's grouping and ACROSS the opposite one:
 *       dy = EDGE SCORES (fora_hip_edge.h) in f64 of (g, v) with flags = 0 and of (v, g) with FORA_SUB_BY_COL -- the products
 *            commute, g is the operand read at the group;
 *       ds = EDGE SOFTMAX backward (fora_hip_edge_softmax.h) of (y[h], dy) with the same flags and scale: the gradient in f64, y
 *            in the caller's type, the output f64;
 *       dq = the along SUBGRAPH PRODUCT (fora_hip_gnn.h) of the k slice with the f64 ds as values: fora_hip_subgraph_propagate
 *            with flags = 0, fora_hip_subgraph_propagate_t with FORA_SUB_BY_COL;
 *       dk = the across product of the q slice with the f64 ds as values;
 *       dv = the across product of the g slice with y[h], in the caller's type, as values.
 *     The order of every sum is the one its contract states; nothing is rounded to f32 in between, and each f32 output is (float)
 *     of its f64 output.  No bit depends on the launch shape, on heads being one call or `heads` calls with heads = 1 on column
 *     slices, on host versus device pointers, or on any option: "attn_short" keeps its meaning and clamp (0 .. 256) and bounds the
 *     groups of BOTH sides that one wave handles; the longer ones go head by head through the kernels of the steps inside the same
 *     call, steered by "softmax_short" and "prop_segs" as those steps are.
 *   - outputs (fora_attn_grads): dq and dk are [nc, heads * d], dv is [nc, heads * dv]; each as f32 and / or f64 with its own
 *     pitch, in host or device memory.  A gradient with both pointers NULL is absent and costs nothing; with dq and dk both absent
 *     dy and ds are never computed and k and v are not read; q is read for dk only.  A node with no edge on the side that sums
 *     gets +0.0.
 *   - non-finite values follow IEEE as in EDGE SOFTMAX backward: nothing is checked, written in place of a result, or counted.
 *     Where a NaN is involved the chained calls agree in NaN-ness only.  scale must be finite.
 *   - the transposition (fora_hip_subgraph_transpose_fetch) is built by the first call that needs it and kept with the subgraph:
 *     every call needs it but one with flags = 0 that wants dq alone, or one over a subgraph of 0 edges.
 *   - info_out (NULL or six int64): the edges; the non-empty groups of at most "attn_short" edges and the longer groups of the
 *     along side; the same two of the across side (both 0 when neither dk nor dv is wanted); 1 if this call built the
 *     transposition.  ms_out (NULL or two doubles): device time of the fused kernels and of the longer groups' path -- each 0
 *     with the option "profile" off.
 *   - lifetime: as EDGE ATTENTION.  The call only reads the held result: the subgraph's arrays, "sparse_generation", the held ids
 *     and words, the contents of both transpositions, the store, the options and fora_timing are untouched.  The plans of both
 *     sides are the forward call's, kept with the subgraph.
 *   - errors: a NULL ctx is answered without touching the GPU (FORA_E_ARG).  No subgraph held, d, dv or heads < 1, heads * d or
 *     heads * dv > 65536, a pitch below its matrix' width (of a gradient: when it is wanted), a type code that is no type, y_type
 *     neither f32 nor f64, an unknown flag bit, a scale that is not finite, grads NULL or all three gradients absent, ycap <
 *     heads * edges, a NULL q, k, v, g or y when there are edges, memory of another GPU: FORA_E_ARG, nothing written.  No device
 *     memory: FORA_E_NOMEM, nothing written.  nc = 0: FORA_OK, nothing launched.  A subgraph of 0 edges: every wanted gradient is
 *     +0.0.  The ctx's stream is idle when the call returns.
 */
#ifndef FORA_HIP_EDGE_ATTENTION_BWD_H
#define FORA_HIP_EDGE_ATTENTION_BWD_H
#include "fora_hip_edge_attention.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the gradients of attention over the held subgraph (the EDGE ATTENTION, BACKWARD contract above) */
int fora_hip_subgraph_attention_bwd(fora_ctx *ctx,
        const void *q /*[nc, heads*d]*/, int q_type, int64_t ldq, const void *k /*[nc, heads*d]*/, int k_type, int64_t ldk,
        const void *v /*[nc, heads*dv]*/, int v_type, int64_t ldv, const void *g /*[nc, heads*dv]*/, int g_type, int64_t ldg,
        const void *y /*[heads][edges]*/, int y_type, uint64_t ycap, int d, int dv, int heads, double scale, int flags,
        const fora_attn_grads *grads, int64_t *info_out /*6 or NULL*/, double *ms_out /*2 or NULL*/);

#ifdef __cplusplus
}
#endif
#endif
