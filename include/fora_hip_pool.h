/* fora_hip_pool.h -- the entry points of libfora_hip.so for max / min pooling over the neighbours of a node in the held subgraph,
 * forward with its arg-max and backward, beside those of fora_hip.h, fora_hip_ext.h, fora_hip_gnn.h, fora_hip_edge.h,
 * fora_hip_edge_softmax.h, fora_hip_edge_attention.h, fora_hip_edge_attention_bwd.h and fora_hip_edge_gat.h: the same library, the
 * same fora_ctx, the same return codes.  Plain C99; statistics leave through out-pointers, so this header declares no struct of
 * its own.
 *
 * SUBGRAPH POOL (fora_hip_subgraph_pool, fora_hip_subgraph_pool_bwd): the element-wise maximum or minimum over a node's
 * neighbours -- the aggregation of GraphSAGE-pool, of PNA's max and min and of PointNet-style layers -- on the held subgraph of
 * fora_hip_sparse_subgraph (nc rows and columns in local ids, sub_ptr / sub_col), with the edge that won, and the gradient.
 *   - groups: with flags & FORA_SUB_BY_COL == 0 the group of node j is the entries e of row j of sub_ptr, in order, the source
 *     node sub_col[e] -- its out-neighbours.  With FORA_SUB_BY_COL it is the positions p of [in_ptr[j], in_ptr[j + 1]) of the
 *     transposition (fora_hip_subgraph_transpose_fetch), in order, the source node in_row[p], the edge e = in_pos[p] -- its
 *     in-neighbours.  Either way an entry is NAMED BY ITS EDGE'S PLACE e IN sub_col, and e ascends inside a group.  A multi-edge
 *     counts as often as it stands; self-loops are included.
 *   - forward, per output element (j, c): t_e = x[src(e)][c] widened to f64 (exact for every element type of PROPAGATE).  The
 *     winner is the FIRST entry of the group under this total order: an entry whose t is NaN stands before every entry whose t
 *     is not; among the others the larger t under IEEE > (the smaller under < with FORA_POOL_MIN), -0.0 and +0.0 being equal;
 *     every tie, among NaNs too, goes to the smaller e.  arg[j][c] = the winner's e as int32; out64[j][c] = the winner's t_e
 *     bit for bit (a leading -0.0 stays -0.0), the quiet NaN 0x7FF8000000000000 where the winner is a NaN; out32 = (float)out64.
 *     An empty group gives out = +0.0 and arg = -1.  The order is total: no bit depends on "sub_short", on the launch shape or on
 *     how a reduction pairs its entries.
 *   - backward, per element (u, c): the ordered sum over the ACROSS group of u -- with flags = 0 the positions p of column u of
 *     the transposition ascending, j = in_row[p], e = in_pos[p]; with FORA_SUB_BY_COL the entries e of row u in order, j =
 *     sub_col[e] -- of term = (arg[j][c] == e) ? widen(g[j][c]) : +0.0: a select, not a multiplication, so a NaN or an infinity of
 *     g reaches only the edge that won.  The terms are added in that order from +0.0 in f64 inside segments of FORA_PROP_SEG =
 *     256 entries, the segments' sums in order -- the order of every product of fora_hip_gnn.h; out32 is out64 rounded once.  An
 *     arg entry that names no edge of its group (-1, an edge of another group) matches nothing and adds nothing; arg is not
 *     validated.  The whole gradient of (j, c) goes to the one edge arg names: ties are not shared.  FORA_POOL_MIN is accepted
 *     and changes nothing here.
 *   - operands and outputs: x / g is [nc, d] of an element type of PROPAGATE at pitch ldx / ldg; out32 and out64, at least one,
 *     [nc, d] at pitch ldo; arg [nc, d] int32 at pitch lda -- an optional output of the forward call, a required input of the
 *     backward one.  Each lives in host memory or in device memory of the ctx's GPU; what lies between the rows stays the
 *     caller's.
 *   - the option "sub_short" splits the groups as it does for the products: a group of at most that many entries (the empty ones
 *     always) is handled by a lane group in one pass; a longer one by a workgroup of its own forward, and through the segments
 *     of the long plan and the combine of PROPAGATE, chunked by "prop_segs", backward.  No bit depends on either.
 *   - the transposition is built by the first call that needs it (forward with FORA_SUB_BY_COL, backward without) and kept with
 *     the subgraph: info_out[0] = 1 then.  info_out (NULL or four int64): the transposition was built by this call; the groups
 *     longer than "sub_short"; the chunks of their path (forward: 1 where there are any -- one launch); x / g lies on the device.
 *     ms_out (NULL or three doubles): device time of the transposition, of the one-pass kernel, of the longer groups' launches
 *     -- each 0 with the option "profile" off.  The calls only read the held result: the subgraph's arrays, "sparse_generation",
 *     the store, the options and fora_timing are untouched.
 *   - errors: a NULL ctx is answered without touching the GPU (FORA_E_ARG).  No subgraph held, a type code that is no type, a
 *     flag bit other than FORA_SUB_BY_COL and FORA_POOL_MIN (FORA_SUB_MEAN among them), d outside 1 .. 65536, a pitch below d,
 *     both outputs NULL, a NULL operand, a NULL arg in the backward call, an arg with 2^31 held edges or more, memory of another
 *     GPU: FORA_E_ARG, nothing written.  No device memory: FORA_E_NOMEM, nothing changed.  nc = 0: FORA_OK, nothing launched.  A
 *     subgraph of 0 edges: forward +0.0 and -1 everywhere, backward +0.0.  The ctx's stream is idle when the calls return.
 */
#ifndef FORA_HIP_POOL_H
#define FORA_HIP_POOL_H
#include "fora_hip_edge_softmax.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FORA_POOL_MIN 4 /* flags: the minimum instead of the maximum; a bit neither FORA_SUB_MEAN nor FORA_SUB_BY_COL uses */

/* ---- max / min pooling over each node's neighbours in the held subgraph (the SUBGRAPH POOL contract above) */
int fora_hip_subgraph_pool(fora_ctx *ctx, const void *x /*[nc, d]*/, int x_type, int d, int64_t ldx, int flags,
                           float *out32 /*or NULL*/, double *out64 /*or NULL*/, int64_t ldo, int32_t *arg /*[nc, d] or NULL*/, int64_t lda,
                           int64_t *info_out /*4 or NULL*/, double *ms_out /*3 or NULL*/);
int fora_hip_subgraph_pool_bwd(fora_ctx *ctx, const void *g /*[nc, d]*/, int g_type, int d, int64_t ldg, int flags,
                               const int32_t *arg /*[nc, d]*/, int64_t lda, float *out32 /*or NULL*/, double *out64 /*or NULL*/, int64_t ldo,
                               int64_t *info_out /*4 or NULL*/, double *ms_out /*3 or NULL*/);

#ifdef __cplusplus
}
#endif
#endif
