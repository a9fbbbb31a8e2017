/* fora_hip_edge.h -- the entry point of libfora_hip.so for values per EDGE of the held subgraph, beside those of fora_hip.h,
 * fora_hip_ext.h and fora_hip_gnn.h: the same library, the same fora_ctx, the same return codes.  Plain C99; statistics leave
 * through out-pointers, so this header declares no struct of its own.
 *
 * EDGE SCORES (fora_hip_subgraph_sddmm): for every edge e of the held subgraph A_S of fora_hip_sparse_subgraph (SUBGRAPH,
 * fora_hip_ext.h; nc rows and nc columns in local ids, sub_ptr / sub_col), e an edge of row j, and every head h,
 *     score[h][e] = < a[j][h*d .. (h+1)*d), b[sub_col[e]][h*d .. (h+1)*d) >
 * -- the dot-product score of the edge j -> sub_col[e]: edge gates, link scores, the scores of an attention layer over the
 * sampled graph, and the gradient of SUBGRAPH PRODUCTS (fora_hip_gnn.h) with respect to their values.
 *   - the bits: the SCORES (SDDMM) contract of fora_hip.h, unchanged, applied to the d columns of the head's slice: the
 *     products (double)a * (double)b are exact; the 64 running sums q_l take the columns c == l (mod 64) of the slice in
 *     ascending c from +0.0; then the tree q_l = q_l + q_{l+o} for o = 32 .. 1; score = q_0.  out32 is out64 rounded once.
 *     No bit depends on the launch shape, on heads being one call or `heads` calls with heads = 1 on column slices, or on
 *     any option.
 *   - operands: a and b are [nc, heads * d]; a is read at the edge's ROW, b at its target sub_col[e].  a_type and b_type are
 *     each an element type of PROPAGATE (FORA_PROP_F32, _BF16, _F16, _E4M3, _E5M2; 3 and 7 are no types), chosen
 *     independently; each matrix lives in host memory or on the ctx's GPU and is read in place at any pitch lda / ldb
 *     >= heads * d.  The rows of a that belong to rows without edges, and the rows of b no edge points at, are never read.
 *   - outputs: out32 (float) and out64 (double), at least one, each [heads][edges] without a pitch -- one head's scores are a
 *     contiguous per-edge array in the order of sub_col, which is what `values` of SUBGRAPH PRODUCTS takes -- in host or
 *     device memory; ocap: the elements each can take, at least heads * edges.
 *   - gradients: for Y = A_S(w) x X, dL/dw_e = <G[row of e], X[sub_col[e]]>: this call with a = G, b = X.  For A_S(w)^T x X:
 *     a = X, b = G.  There is no direction flag.
 *   - lifetime: the call works on the held subgraph and takes no row_ptr; no subgraph held: FORA_E_ARG.  It only reads the
 *     held result: the subgraph's arrays and its transposition, "sparse_generation", the held ids and words, the store, the
 *     options and fora_timing are untouched; nothing is planned on the host and nothing is kept.
 *   - info_out (NULL or four int64): the edges; the workgroups launched; a lies on the device; b lies on the device.
 *     ms_out (NULL or one double): device time of the kernel -- 0 with the option "profile" off.
 *   - errors: a NULL ctx is answered without touching the GPU (FORA_E_ARG).  d < 1, heads < 1, heads * d > 65536, a pitch
 *     below heads * d, both outputs NULL, a type code that is no type, ocap < heads * edges, a NULL operand, memory of
 *     another GPU: FORA_E_ARG, nothing written.  No device memory: FORA_E_NOMEM, nothing changed.  nc = 0 or a subgraph of
 *     0 edges: FORA_OK, nothing launched or written.  The ctx's stream is idle when the call returns.
 */
#ifndef FORA_HIP_EDGE_H
#define FORA_HIP_EDGE_H
#include "fora_hip_gnn.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- scores per edge of the held subgraph (the EDGE SCORES contract above) */
int fora_hip_subgraph_sddmm(fora_ctx *ctx, const void *a /*[nc, heads*d]*/, int a_type, int64_t lda,
                            const void *b /*[nc, heads*d]*/, int b_type, int64_t ldb, int d, int heads,
                            float *out32 /*or NULL*/, double *out64 /*or NULL*/, uint64_t ocap,
                            int64_t *info_out /*4 or NULL*/, double *ms_out /*1 or NULL*/);

#ifdef __cplusplus
}
#endif
#endif
