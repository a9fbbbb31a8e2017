/* fora_hip_gnn.h -- entry points of libfora_hip.so for message passing on the held subgraph, beside those of fora_hip.h and
 * fora_hip_ext.h: the same library, the same fora_ctx, the same return codes.  Plain C99; statistics leave through
 * out-pointers, so this header declares no struct of its own.
 *
 * SUBGRAPH PRODUCTS (fora_hip_subgraph_propagate, fora_hip_subgraph_propagate_t, fora_hip_subgraph_transpose_fetch): the held
 * subgraph A_S of fora_hip_sparse_subgraph (SUBGRAPH, fora_hip_ext.h) -- nc rows and nc columns in local ids, sub_ptr / sub_col --
 * times a dense matrix, in both directions: one GCN / SAGE aggregation over the nodes of a mini-batch and its gradient.
 *   - fora_hip_subgraph_propagate: out = A_S x X.  x is [nc, d] at pitch ldx; out[j] = sum over the edges e of row j of the
 *     held subgraph, in the order of sub_col, of w_e * x[sub_col[e]] -- the aggregation over the out-neighbours of cols[j]
 *     inside the batch.  A multi-edge counts as often as it stands; self-loops are included.
 *   - fora_hip_subgraph_propagate_t: out = A_S^T x G.  g is [nc, d] at pitch ldg; out[v] = sum over the edges e with
 *     sub_col[e] == v, in ascending e, of w_e * g[row(e)] -- the aggregation over in-neighbours, and the gradient of the forward
 *     call with respect to x when g is the gradient with respect to its output.  values is still indexed by the edge's place
 *     in sub_col.
 *   - weights: values == NULL: every w_e is 1.0.  Otherwise w_e = (double)values[e], val_type FORA_PROP_F32 or FORA_PROP_F64,
 *     one value per edge of the subgraph in the order of sub_col (gather graph edge weights with sub_eid); values lives in
 *     host memory or on the ctx's GPU.  flags: FORA_SUB_MEAN divides the finished f64 sum of an output row once, in f64, by
 *     (double) the number of its terms; a row without terms is +0.0.  FORA_SUB_MEAN together with values, or any other flag
 *     bit: FORA_E_ARG.
 *   - operands and outputs: x_type / g_type is an element type of PROPAGATE (FORA_PROP_F32, _BF16, _F16, _E4M3, _E5M2; 3 and 7
 *     are no types: FORA_E_ARG), any pitch >= d, host memory or device memory of the ctx's GPU read in place.  out32 (float)
 *     and out64 (double), at least one, [nc, d] at pitch ldo (both with the same pitch), in host or device memory; what lies
 *     between the rows stays the caller's.
 *   - the bits: per output row, term_e = w_e * widen(x) is one unfused f64 multiply; the terms are added in entry order from
 *     +0.0 inside segments of FORA_PROP_SEG = 256 entries; the segments' sums are added in order; then the MEAN division;
 *     out32 is out64 rounded once.  No bit depends on any option ("sub_short", "prop_segs", "propt_lds_cap"), on the launch
 *     shape, on chunking, or on the order in which the device meets the edges.  The option "sub_short" (default 256, clamped
 *     to 0 .. 256; readable from the environment like the other non-schedule knobs) says up to how many entries an output
 *     row is summed and written by the one-pass kernel; longer rows take the kernels of PROPAGATE inside the same call; 0:
 *     every non-empty row does.
 *   - fora_hip_subgraph_transpose_fetch copies the transposition out: in_ptr nc + 1 int64 offsets, in_row (int32) the local
 *     row an entry came from, in_pos (int64) the edge's place in sub_col -- column by column, ascending in_pos inside a
 *     column.  Each array goes to pageable host memory or to device memory of the ctx's GPU, under the rules of
 *     fora_hip_sparse_subgraph_fetch; any of the three may be NULL; cap = the entries in_row and in_pos can take, smaller than
 *     the edges: FORA_E_ARG.  The call builds the transposition if it is not there.
 *   - lifetime: the calls work on the held subgraph and take no row_ptr; no subgraph held: FORA_E_ARG.  The transposition
 *     (built by the first transposed call or by the fetch: info_out[0] = 1, later calls 0) and the plans of the longer rows
 *     are kept with the subgraph and end where it ends or is built again.  The calls only read the held result: the
 *     subgraph's arrays, "sparse_generation", the held ids and words, the transposition of the held rows, the store, the
 *     options and fora_timing are untouched.
 *   - info_out (NULL or four int64): the transposition was built by this call; the output rows longer than "sub_short";
 *     the chunks of their path; x lies on the device.  ms_out (NULL or three doubles): device time of the transposition, of
 *     the one-pass kernel, of the longer rows' launches -- each 0 with the option "profile" off.
 *   - errors: a NULL ctx is answered without touching the GPU (FORA_E_ARG).  d < 1, a pitch below d, both outputs NULL,
 *     a NULL operand, memory of another GPU: FORA_E_ARG, nothing written.  No device memory: FORA_E_NOMEM, nothing changed.
 *     nc = 0: FORA_OK, nothing launched.  A subgraph of 0 edges: every output row is written as +0.0.  The ctx's stream
 *     is idle when the calls return.
 */
#ifndef FORA_HIP_GNN_H
#define FORA_HIP_GNN_H
#include "fora_hip_ext.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FORA_SUB_MEAN 1 /* flags: every output row divided by the number of its terms */

/* ---- message passing on the held subgraph (the SUBGRAPH PRODUCTS contract above) */
int fora_hip_subgraph_propagate(fora_ctx *ctx, const void *x /*[nc, d]*/, int x_type, int d, int64_t ldx, int flags,
                                const void *values /*edges or NULL*/, int val_type, float *out32 /*or NULL*/, double *out64 /*or NULL*/,
                                int64_t ldo, int64_t *info_out /*4 or NULL*/, double *ms_out /*3 or NULL*/);
int fora_hip_subgraph_propagate_t(fora_ctx *ctx, const void *g /*[nc, d]*/, int g_type, int d, int64_t ldg, int flags,
                                  const void *values /*edges or NULL*/, int val_type, float *out32 /*or NULL*/, double *out64 /*or NULL*/,
                                  int64_t ldo, int64_t *info_out /*4 or NULL*/, double *ms_out /*3 or NULL*/);
int fora_hip_subgraph_transpose_fetch(fora_ctx *ctx, int64_t *in_ptr /*nc+1 or NULL*/, int32_t *in_row /*or NULL*/,
                                      int64_t *in_pos /*or NULL*/, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif
