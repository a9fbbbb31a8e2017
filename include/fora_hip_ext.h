/* fora_hip_ext.h -- entry points of libfora_hip.so beside those of fora_hip.h: the same library, the same fora_ctx, the same
 * return codes.  Plain C99; statistics leave through out-pointers, so this header declares no struct of its own.
 *
 * SUBGRAPH (fora_hip_sparse_subgraph, fora_hip_sparse_subgraph_fetch): the subgraph the graph induces on the columns of a
 * compacted held result -- the edges of the graph among the nodes of a mini-batch, for message passing on the sampled node set
 * (ShaDow, GraphSAINT, any PPR-sampled GNN).  The library holds the graph as fora_hip_set_graph took it, and U with its bitmap
 * from the compaction (COLUMNS, fora_hip.h): only the out-edges of the nodes of U are read, never all m edges.
 *   - fora_hip_sparse_subgraph works on a COMPACTED held result (fora_hip_sparse_compact; row_ptr is validated exactly as in
 *     PROPAGATE).  Let U = cols with nc entries.  It builds one CSR over U in local ids and keeps it on the device: for j in
 *     [0, nc), row j is the out-row of node U[j] in the graph's own order (the order of col as given to fora_hip_set_graph); an
 *     edge is kept exactly when its target is in U; multi-edges and self-loops are kept as they stand.  sub_col holds the
 *     target's rank in U, sub_eid the edge's position in the graph's col array (for gathering edge weights or features),
 *     sub_ptr nc + 1 int64 offsets with sub_ptr[nc] = *edges_out (required).  *scanned_out = the sum of the out-degrees of the
 *     nodes of U, the edges the call read; *ms_out = the device time of the call's kernels (0 with the option "profile" off).
 *   - fora_hip_sparse_subgraph_fetch copies the held subgraph out, each array to pageable host memory or to device memory on
 *     the ctx's GPU (memory of another GPU is FORA_E_ARG); any of the three may be NULL.  cap = the entries sub_col and sub_eid
 *     can take.  cap smaller than the edges, or no subgraph held: FORA_E_ARG.
 *   - the subgraph ends wherever the compacted held result ends: every call that makes a new held result (fora_hip_store_take
 *     included), fora_hip_sparse_clear, fora_hip_set_graph, fora_hip_destroy.  Building it does NOT move "sparse_generation",
 *     does not drop the transposition, and leaves the held ids, words and columns, the store, a held sweep profile, the walk
 *     index, the options, the FORA parameters and fora_timing untouched: it only reads the held result.  A second build on the
 *     same held result gives the same arrays.  The ctx's stream is idle when both calls return.
 *   - a NULL ctx is answered without touching the GPU (FORA_E_ARG).  No held result, a held result that is not compacted, a
 *     row_ptr that is not the held result's, a NULL edges_out: FORA_E_ARG, nothing changed.  No device memory: FORA_E_NOMEM,
 *     nothing changed.  A device failure behind the first launch leaves no subgraph held and the held result as it was.
 *     nc = 0: FORA_OK, 0 edges, nothing launched (sub_ptr is the one entry 0).
 *   - integers only.  No bit depends on the option "sub_span" (the scanned edges one workgroup of the count and write passes
 *     takes: a power of two from 256 to 8192, other values are clamped and rounded down to one; readable from the environment
 *     like the other non-schedule knobs), on the launch shape, on nq, or on the order in which the device meets the edges.
 */
#ifndef FORA_HIP_EXT_H
#define FORA_HIP_EXT_H
#include "fora_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the induced subgraph of a compacted held result (the SUBGRAPH contract above) */
int fora_hip_sparse_subgraph(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq, int64_t *edges_out /*required*/,
                             uint64_t *scanned_out /*or NULL*/, double *ms_out /*or NULL*/);
int fora_hip_sparse_subgraph_fetch(fora_ctx *ctx, int64_t *sub_ptr /*nc+1 or NULL*/, int32_t *sub_col /*or NULL*/,
                                   int64_t *sub_eid /*or NULL*/, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif
