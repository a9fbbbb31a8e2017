/*
 * fora_hip.h -- C ABI of the MI355X-native FORA SSPPR engine (libfora_hip.so).
 *
 * The reference (wangsibovictor/fora) exposes no plugin / FFI interface; its
 * seams are C++ free functions that read and write global state from one thread
 * (SURVEY.md 8b).  Each entry point below names the reference seam it replaces.
 * Conventions: plain C types only, caller-allocated outputs, return 0 on success
 * or a negative FORA_E_* code (never throws, never exit()s), one ctx per GPU, a
 * ctx is used by one host thread at a time.  All host pointers are ordinary
 * pageable memory; the library copies.
 *
 * NUMERIC CONTRACT.  residue / reserve / ppr live on the device as unsigned 2^-62 fixed point
 * (1.0 == FORA_FIX_ONE), so every accumulation is an exact, order-independent integer add:
 *   - results are bit-reproducible (same inputs, same seed -> same bits, whatever the batch size, the bucket
 *     layout or the GPU count) and equal oracle/fora_twin.c bit for bit;
 *   - mass is conserved EXACTLY: after the push sum(reserve) + sum(residue) == FORA_FIX_ONE, after the refinement
 *     sum(ppr) == FORA_FIX_ONE (fora_query_stats.ppr_sum_fix); walk j of a residue node carries floor(r / num_s_rw)
 *     plus one more unit for j < r mod num_s_rw;
 *   - a pop keeps floor(alpha * r) -- alpha enters as floor(alpha * 2^62) -- and every out-edge gets
 *     floor((r - keep) / outdeg); the division remainder (< outdeg units of 2^-62 = 2.2e-19) stays in the RESERVE of
 *     the popped node, where the reference's f64 `((1-alpha)*r)/outdeg` (algo.h:1002) rounds instead;
 *   - the threshold test residue/outdeg >= rmax (algo.h:1012) is residue >= ceil(rmax * 2^62) * outdeg;
 *   - double-typed outputs (ppr_out, scores, rsum) are value * 2^-62: absolute resolution 2.2e-19, i.e. at least
 *     9 significant digits for any entry >= 1/n of a graph of up to 2^31 nodes.
 * ERROR BOUND of ppr_out against exact PPR pi(s, .) (power iteration, query.h:1192-1224): the FORA guarantee the
 * parameters of algo.h:455-463 encode, |ppr - pi| <= epsilon * pi for every pi >= 1/n with probability
 * 1 - 1/n; the fixed point adds at most (pops + relaxations + walks) * 2^-62 < 1e-8 * that bound.  Checked at
 * n = 281 904 in tests/test_hip_parity_gpu.py::test_full_size_webstanford_properties (L-inf <= 2e-5).
 * RNG CONTRACT, version 2 (replaces the time(0)-seeded Boost engines of algo.h:105-122): Philox4x32-10, key = seed,
 * one call per two steps, counter = (start node, walk# lo32, walk# bits 32..47 | round << 16 | (step/2 & 255) << 24,
 * stream ^ (step >> 9) * 0x9E3779B9), stream = the query's source id (FORA_STREAM_INDEX for index walks).
 * Version 1 (round 1) lacked the (step >> 9) term; walks of up to 512 steps are identical in both.
 * Monte-Carlo walks (fora_hip_montecarlo_batch): source s runs W walks, W = the number of integers i >= 0 with
 * (double)i < omega_mc (the reference's `for (unsigned long i = 0; i < config.omega; i++)`, query.h:24); walk j < W is
 * the walk above with start = s, stream = s, round = 0, walk# j, zero-hop walks allowed (random_walk, algo.h:124-142),
 * i.e. it ends where orc_walk(g, seed, s, 0, s, j) and fora_hip_walks(stream s, round 0, no_zero_hop 0, start s, j) end.
 * It carries floor(2^62 / W) + (j < 2^62 mod W) units to its endpoint, so sum(ppr) == FORA_FIX_ONE exactly; the
 * reference's cnt / omega differs from that by a factor omega / W, between 1 - 1/omega and 1.
 * BACKWARD PUSH (fora_hip_bwdpush_batch; reverse_local_update_linear, algo.h:703-751) works at its own fixed point,
 * 1.0 == FORA_BWD_FIX_ONE == 2^60.  Target t starts from r = e_t * 2^60, p = 0; thr = floor(rmax * 2^60), and a node
 * pops iff r[v] > thr (the reference's `> myeps`, algo.h:743).  The push is level-synchronous: at each level every v
 * of F = {v : r[v] > thr} pops at the same moment -- x = r[v], r[v] = 0, keep = floor(x * alpha62 / 2^62) with
 * alpha62 = floor(alpha * 2^62) (the forward push's alpha), p[v] += keep, y = x - keep -- and every in-edge u -> v of the
 * CSR (duplicates each with its own share, self loops dropped as they are in the CSR) adds floor(y / outdeg(u)) to
 * r[u]; all increments land after all pops of the level, and the push stops when F is empty.  The reference's FIFO
 * order is not reproduced (its `break` on `< myeps`, algo.h:725, never fires: a queued residue only grows).
 * Counters: pops, relaxations (in-edges traversed at every pop) and levels (levels with a non-empty F).
 * Backward residues are not probability mass: a node under the threshold can collect (1 - alpha) * max r in one level,
 * so every r stays below max(1, rmax / alpha) and every BiPPR estimate below 1 + max(1, rmax / alpha).  A u64 at 2^60
 * holds values below 16: an (alpha, rmax) with 1 + max(1, rmax / alpha) >= 16 is FORA_E_ARG.
 * BIPPR (fora_hip_bippr_batch; bippr_query, query.h:71-124; bippr_query_topk :126-193): bippr_setting (algo.h:442-447)
 * in the reference's operand order with delta = pfail = 1/n, m = m_attr:
 * rmax = epsilon*sqrt(m*1.0*delta/3.0/log(2.0/pfail)); rmax *= rmax_scale; omega = rmax*3*log(2.0/pfail)/delta/epsilon/epsilon;
 * W = ceil(omega), FORA_E_ARG unless 1 <= W < 2^48.  The ctx's alpha and seed are used, its FORA rmax / omega are left
 * untouched.  c = the walk slab at 2^-62: walks j < W with start = stream = s, round 0, each carrying
 * floor(2^62 / W) + (j < 2^62 mod W) units (the Monte-Carlo slab of fora_hip_montecarlo_batch, with W walks).  For every
 * node i (a backward push to target i at rmax, giving p_i, r_i): ppr[i] = p_i[s] + sum_v floor(c[v] * r_i[v] / 2^62), at
 * 2^60, each term floored on its own from the 128-bit product and the terms added as integers.  With rmax >= 1 nothing
 * pops and ppr[i] = floor(c[i] / 4) (the reference's else branch, query.h:114-119).  A dangling source keeps the
 * reference's bias: every walk stops at s and no in-edge reaches s, so ppr = keep(2^60) at s and 0 elsewhere.  Double
 * outputs are value * 2^-60; sum(ppr) (ppr_sum_fix) is NOT conserved (an estimate, not a distribution).
 * TARGETED BIPPR (fora_hip_bippr_targets_batch): the BIPPR estimate for nq sources and a caller's list of nt targets, with
 * nt backward pushes per call instead of n.  Parameters, W and their bounds, the walk slab of a source and the use of the
 * ctx's alpha and seed are those of BIPPR above; the ctx's FORA rmax / omega stay untouched.  est_fix_out[i*nt + j] is, bit
 * for bit, the word fora_hip_bippr_batch writes to ppr_fix_out[i*n + targets[j]] for the same ctx, epsilon and rmax_scale:
 * p_t[s] + sum_v floor(c_s[v] * r_t[v] / 2^62) at 2^60 with s = sources[i], t = targets[j]; est_out is that word * 2^-60.
 * The batch size, the tier ("bwd_lds_cap"), the chunking ("bwd_chunk") and the way the combine splits its work
 * ("tgt_lanes", "tgt_span") change no bit.  With few targets a small rmax_scale moves work from the walks (W shrinks in
 * proportion) into the nt pushes.
 *   - targets come in the caller's order, in any order; duplicate targets give duplicate columns, duplicate sources
 *     duplicate rows; nt may exceed n.  A target without in-edges, or a dangling one, is an ordinary target.
 *   - a dangling source gives keep(2^60) = floor(2^60 * alpha62 / 2^62) in the columns whose target is s and 0 elsewhere
 *     (the bias above); rmax >= 1 gives floor(c_s[t] / 4).
 *   - stats, per source: n_walks = W, rmax_used, dangling_source, ppr_sum_fix = the sum of that row's nt words (u64,
 *     wrapping); every other field 0.  *bwd: targets = nt; pops, relax and entries summed over the nt pushes, a target
 *     listed twice counted twice; global_targets, levels, chunks and the three times as for fora_hip_bippr_batch.
 *     fora_timing: walks, walk_steps, walk_ms.
 *   - nq == 0 or nt == 0: FORA_OK, nothing is written to the estimates, the stats of the sources are filled
 *     (ppr_sum_fix 0), *bwd is all zero: no push and no walk runs.
 *   - NULL ctx (answered without touching the GPU), NULL sources with nq > 0, NULL targets with nt > 0, an id outside
 *     [0, n), epsilon <= 0, rmax_scale <= 0 or not finite, an (alpha, rmax) out of the fixed point's range: FORA_E_ARG.
 *     No device memory for a batch's nb x nt estimate block: FORA_E_NOMEM, the ctx still usable.
 *   - a held sparse result, the walk index, the options and the FORA parameters are left untouched.
 * SPARSE RESULTS (fora_hip_query_sparse_batch, fora_hip_sparse_fetch, fora_hip_sparse_clear).  The query is
 * fora_hip_query_batch's: same push, same walks, same batching, same dangling-source fast path, same fora_query_stats,
 * same bits in the ppr slabs.  Only what leaves the device differs: a CSR over the call's sources, compacted on the GPU.
 *   - thr_fix = max(1, ceil(threshold * 2^62)), threshold * 2^62 being the exact ldexp of the double; threshold <= 0
 *     means 1 (every non-zero entry); threshold > 1 or NaN is FORA_E_ARG.  Node v of row i is kept iff
 *     ppr_fix[i][v] >= thr_fix: the test is made on the fixed-point word, never on a double.  sum(ppr) == FORA_FIX_ONE,
 *     so a row has at most floor(2^62 / thr_fix) entries, whatever the graph.
 *   - row i belongs to sources[i], in the caller's order; duplicate sources give duplicate rows; a dangling source gives
 *     the single entry (s, FORA_FIX_ONE); inside a row the ids ascend; row_ptr[0] == 0, row_ptr[nq] == entries.
 *   - fix is the raw word and vals[j] == ldexp((double)fix[j], -62), the value the dense ppr_out holds for that node.
 *   - the result lives in device memory owned by the ctx, outside the query workspace.  It stays valid until the next
 *     fora_hip_query_sparse_batch or fora_hip_seeds_sparse_batch or one of their top-k forms (whatever that call returns),
 *     fora_hip_sparse_clear, fora_hip_set_graph or fora_hip_destroy; every other entry point (queries, top-k, baselines, set_option, set_batch, a bucket retry of a
 *     later call) leaves it untouched.  A failed sparse call leaves no result.
 *   - fora_hip_sparse_fetch may be called any number of times.  Each output pointer may be pageable host memory or device
 *     memory on the ctx's GPU (a device destination is written by the device, never staged through the host).  The ctx's
 *     stream is synchronised before the call returns, so another stream may read a device destination at once.
 *     cap < entries, or no held result: FORA_E_ARG and nothing is written.
 *   - NULL ctx (answered without touching the GPU), NULL row_ptr, bad nq / sources, with_idx without an index:
 *     FORA_E_ARG.  No device memory for the result: FORA_E_NOMEM, no result held, the ctx still usable.
 * SEED SETS (fora_hip_query_seeds_batch): PPR that restarts on a weighted SET of nodes, pi(w, .) = sum_j w_j * pi(s_j, .), one
 * row per set.  Every seed the call needs runs once as an ordinary query of fora_hip_query_batch (same push, same walks, same
 * batching, same dangling-source fast path); the rows are folded on the GPU, in fixed point, before anything leaves it.
 *   - set g is seeds[set_ptr[g] .. set_ptr[g+1]), k_g >= 1 seeds in the caller's order.  Duplicate seeds inside a set are
 *     separate terms, the same seed may appear in many sets, duplicate sets give duplicate rows.
 *   - weights == NULL (uniform): seed j of a set (0-based) gets wfix_j = floor(2^62 / k_g) + (j < 2^62 mod k_g), so
 *     sum(wfix) == 2^62 exactly.
 *   - weights given (set_ptr[ns] of them, beside the seeds): every weight finite and >= 0, the set's sum S > 0 (and finite), S
 *     added left to right in doubles; wfix_j = (uint64_t)ldexp(w_j / S, 62) -- the ldexp is exact, the cast floors, every
 *     wfix_j <= 2^62; sum(wfix) <= 2^62 up to the rounding of the k_g divisions and of the adds of S (2^-53 relative each,
 *     2^9 units: sum(wfix) <= 2^62 + 2^10 k_g; <= 2^62 where S and the quotients are exact).
 *   - row_g[v] = sum_j floor(wfix_j * x_j[v] / 2^62), x_j being the row fora_hip_query_batch_fix writes for seeds[j] with the same
 *     ctx state (parameters, seed, with_idx, options, --balanced): each term floored on its own from the 128-bit product, the
 *     terms added as integers.  The value is at 2^-62; ppr_out is the word * 2^-62.  A dangling seed contributes exactly wfix_j
 *     at v = s_j (its row is FORA_FIX_ONE at s).  A singleton set with uniform weight gives x unchanged.
 *   - row_sum_fix_out[g] = sum_v row_g[v] <= sum(wfix) (bounded above: exactly 2^62 for uniform weights): the combine creates
 *     no mass beyond the weights; the mass lost is at most one unit per non-zero term.
 *   - no bit depends on the batch size, on which batch a seed lands in, on the option "seeds_dedup" (1, default: a seed id runs
 *     once per call; 0: every listed seed takes a slot of its own) or on any knob the environment can set: the rows x_j have
 *     that property and the combine is integer adds.
 *   - top-k: 1 <= k <= min(1024, n), or k == 0 for none; score descending, ties by ascending id, padded with (0, 0.0), as
 *     fora_hip_topk_batch; taken from row_g, scores = word * 2^-62.
 *   - stats: seeds = set_ptr[ns]; distinct = distinct seed ids; queries = single-source queries run; dangling = listed seeds
 *     without out-edges (they never take a slot); batches; combine_ms.  fora_timing folds the underlying queries exactly as
 *     fora_hip_query_batch would.
 *   - ns == 0: FORA_OK, nothing is written, *st is all zero.
 *   - NULL ctx (answered without touching the GPU), ns < 0, NULL set_ptr or seeds with work to do, set_ptr[0] != 0, a decreasing
 *     set_ptr, an empty set, a seed id outside [0, n), a bad weight or a zero sum, with_idx without an index, a bad k:
 *     FORA_E_ARG.  No device memory for the ns x n accumulator block: FORA_E_NOMEM, the ctx still usable; the caller splits
 *     the call.
 *   - a held sparse result, the walk index, the options and the FORA parameters are left untouched.
 * SEED SETS, SPARSE (fora_hip_seeds_sparse_batch): the rows of SEED SETS leave as the CSR of SPARSE RESULTS.  row_g is exactly the
 * row fora_hip_query_seeds_batch defines (sets, weights, wfix, duplicates, dangling seeds, every word); the threshold and thr_fix
 * are those of SPARSE RESULTS, applied to row_g -- AFTER the sum: a node whose every term is under thr_fix is kept when their
 * sum reaches it, which no merge of per-seed thresholded rows can give.
 *   - row g keeps {v : row_g[v] >= thr_fix}, ids ascending, words unchanged.  The result is the held sparse result of SPARSE
 *     RESULTS: a call replaces whatever sparse result was held (whatever becomes of the call), fora_hip_sparse_fetch copies it to
 *     host or device arrays, fora_hip_sparse_clear drops it.  row_sum_fix_out[g] is the sum over the WHOLE row, as in SEED SETS.
 *   - a uniform singleton set [s] gives the entries of fora_hip_query_sparse_batch for s, word for word (a dangling s: (s, 2^62)).
 *   - no bit depends on what SEED SETS names, nor on the option "seeds_rows" (rows of the accumulator block compacted at a time,
 *     default 256, at least 1; with an odd n it is rounded up to even so that every chunk of rows starts 16-byte aligned).
 *   - stats: *st as in SEED SETS, *sp as in SPARSE RESULTS with batches = chunks of rows compacted.  ns == 0: FORA_OK,
 *     row_ptr[0] = 0, an empty result held, both stats all zero.
 *   - errors: those of SEED SETS, plus a NULL row_ptr and a bad threshold (FORA_E_ARG).  No device memory for the accumulator
 *     block or the result: FORA_E_NOMEM, nothing held, the ctx still usable.
 *   - a held sweep result, the walk index, the options and the FORA parameters are left untouched; fora_timing as in SEED SETS.
 * SPARSE RESULTS, TOP-K (fora_hip_query_sparse_topk_batch, fora_hip_seeds_sparse_topk_batch): the rows of SPARSE RESULTS and of
 * SEED SETS, SPARSE cut down to their k largest entries on the GPU.  Row i is the row fora_hip_query_sparse_batch defines (for
 * seed sets: row_g of SEED SETS, SPARSE, thresholded after the sum); its support is {v : word[v] >= thr_fix}, thr_fix from
 * `threshold` exactly as there, len = |support|.  Everything is an integer.
 *   - k is an int64_t, k >= 1; any other k is FORA_E_ARG.  k is checked beside the threshold, behind the point where the call
 *     ends the held sparse result: a bad k, like a bad threshold (or a NULL row_ptr), leaves NO result held -- the one held
 *     before the call is gone and "sparse_generation" has moved.
 *   - len <= k: the row is held unchanged.  Otherwise the row keeps the k entries of the support that come first in the strict
 *     order (word descending, id ascending); ids inside a row are distinct, so any correct selection gives the same arrays.
 *   - the kept entries are held in ASCENDING ID order, words unchanged: what every consumer of the held result requires, and a
 *     row still lists a node at most once.
 *   - a dangling source gives the single entry (s, FORA_FIX_ONE) for every k; a uniform singleton seed set [s] gives the
 *     single-source top-k row for s, word for word.
 *   - row_ptr is the prefix sum of min(len, k), one entry per dangling row.
 *   - the result IS the held sparse result and replaces what was held: fora_hip_sparse_fetch, _clear, _propagate, _propagate_t
 *     and _transpose_fetch work on it unchanged, "sparse_generation" moves as for the plain calls; a held sweep profile, the
 *     walk index, the options and the FORA parameters are untouched.
 *   - no bit depends on the batch size, on the batch a row lands in, on "seeds_rows" or "seeds_dedup", on the tier a row took,
 *     or on the options "topk_lds_cap" (candidates of a cut row that one workgroup selects in LDS at most; 0: every cut row is
 *     selected from global memory) and "topk_cand" (entries of the candidate scratch a batch is compacted into chunk by chunk;
 *     0: by free memory; at least the longest row, a row is never split).  With k >= the longest support row_ptr, ids and fix
 *     equal those of the plain call word for word.
 *   - stats: *stats / *st as for the plain calls.  *sp: entries = row_ptr[nq], max_row = the longest HELD row, compact_ms = the
 *     count and candidate passes.  *tk: support / max_support = sum and max of len over the live rows, k, cut_rows (len > k),
 *     lds_rows / global_rows (cut rows per tier), chunks (candidate chunks written), select_ms.  row_sum_fix_out stays the sum
 *     over the WHOLE row, as in SEED SETS.
 *   - errors: those of the plain calls.  No device memory for the candidates or the result: FORA_E_NOMEM, nothing held, the
 *     ctx still usable.
 * SWEEP CUT (fora_hip_sweep_batch, fora_hip_sweep_fetch, fora_hip_sweep_clear): local clustering by a sweep over ppr / degree
 * (Andersen-Chung-Lang), computed on the GPU from the rows of a query.  The query is fora_hip_query_batch's: same push, same
 * walks, same batching, same dangling-source fast path, same fora_query_stats, same bits in the ppr slabs.  Only what is derived
 * from a row is new.  Row i belongs to sources[i]; everything below is an integer.
 *   - thr_fix = max(1, ceil(threshold * 2^62)), as for the sparse results: threshold <= 0 means 1, threshold > 1 or NaN is
 *     FORA_E_ARG.  Support = {v : ppr_fix[i][v] >= thr_fix}; dangling nodes are ordinary members; a dangling source's row is the
 *     single entry (s, 2^62).
 *   - key(v) = floor(ppr_fix[v] / max(outdeg(v), 1)), a u64.  The sweep order sorts the support by key descending, ties by
 *     ascending id; ids inside a row are distinct, so the order is strict and any correct sort gives the same bits.  The key is a
 *     quotient and not a cross-multiplied compare of ppr_a * deg_b with ppr_b * deg_a: one u64 per node is what a radix or a
 *     bitonic sort takes, and the floor loses less than one unit of 2^-62 of ppr per unit of degree.
 *   - len = |support|; L = len if max_size <= 0, else min(len, max_size).  The profile of the row has L entries, order[0..L);
 *     support nodes past L count as outside.
 *   - for the prefix S_j = order[0..j], j < L: vol[j] = sum of outdeg(u) over S_j (the real out-degree: a dangling node adds 0);
 *     cut[j] = number of CSR edges u -> v with u in S_j and v not in S_j (every stored duplicate counts once; the CSR holds no
 *     self loops); den[j] = min(vol[j], nnz - vol[j]) with nnz = row_ptr[n] of fora_hip_set_graph (not m_attr).  On a symmetric
 *     CSR cut / den is the usual conductance; on a directed one it is the out-cut over the out-volume.
 *   - best = the j + 1 that minimises cut[j] / den[j] over the prefixes with den[j] > 0, compared exactly as
 *     cut_a * den_b < cut_b * den_a on the 128-bit products, ties to the smaller prefix.  No prefix with den > 0 (an empty row, a
 *     dangling source, a support of dangling nodes only, a support whose every prefix has vol == nnz): best = 0, cut = vol = den = 0, conductance = 1.0.
 *     Otherwise cut, vol, den are those of the best prefix and conductance = (double)cut / (double)den: each integer converted
 *     to f64, then one IEEE division.
 *   - no bit depends on the batch size, on which batch a source lands in, on the push layout, on any knob the environment can
 *     set, or on the options "sweep_lds_cap" (entries of a sort tile: a row that fits one is sorted by one workgroup in LDS, a
 *     longer one takes the global tier; 0: every row does) and "sweep_rows" (rows whose rank maps are live at a time).
 *   - the profile (order, cut, vol per row, rows in the caller's order, row_ptr = prefix sums of L) lives in device memory owned
 *     by the ctx, outside the query workspace.  It stays valid until the next fora_hip_sweep_batch or fora_hip_seeds_sweep_batch (whatever that call returns),
 *     fora_hip_sweep_clear, fora_hip_set_graph or fora_hip_destroy; every other entry point leaves it untouched.  A sweep call
 *     leaves a held sparse result, the walk index, the options and the FORA parameters untouched.
 *   - fora_hip_sweep_fetch: any pointer may be NULL; each may be pageable host memory or device memory on the ctx's GPU.
 *     cap < entries (row_ptr[nq]), or no held result: FORA_E_ARG and nothing is written.  The members of row i's best cluster
 *     are ids[row_ptr[i] .. row_ptr[i] + rows[i].best).
 *   - stats: entries = sum of len, max_row = the largest len, thr_fix, edges = out-edges scanned (sum of outdeg over the
 *     profiles), batches, global_rows = rows sorted on the global tier, and the device times of the three stages.
 *   - NULL ctx (answered without touching the GPU), NULL row_ptr, bad nq / sources, with_idx without an index: FORA_E_ARG.  No
 *     device memory: FORA_E_NOMEM, nothing held, the ctx still usable.  nq == 0: FORA_OK, row_ptr[0] = 0, an empty result held.
 * SEED SETS, SWEPT (fora_hip_seeds_sweep_batch): seed-set expansion -- the SWEEP CUT contract applied to the rows of SEED SETS.
 * row_g is exactly the row fora_hip_query_seeds_batch defines; it is swept as an ordinary row: thr_fix, support, key, order, L,
 * cut, vol, den, best prefix, ties and conductance are those of SWEEP CUT, with row_g in the place of ppr_fix[i].
 *   - there is no special case for dangling seeds: they are members of the support like any node.  A set of dangling seeds only
 *     has those seeds as its support and vol = 0 everywhere, hence best = 0 and conductance = 1.0.
 *   - the result is the held profile of SWEEP CUT: a call replaces whatever profile was held (whatever becomes of the call),
 *     fora_hip_sweep_fetch copies it, fora_hip_sweep_clear drops it.
 *   - a uniform singleton set [s] gives the fora_sweep_row and the profile of fora_hip_sweep_batch for s, word for word (a
 *     dangling s: len 1, best 0, the profile entry (s, 0, 0)).
 *   - no bit depends on what SEED SETS and SWEEP CUT name, nor on the option "seeds_rows" (rows of the accumulator block
 *     compacted and sorted at a time; "sweep_rows" keeps bounding the rank maps inside such a chunk).
 *   - stats: *st as in SEED SETS, *sw as in SWEEP CUT with batches = chunks of rows.  ns == 0: FORA_OK, row_ptr[0] = 0, an empty
 *     result held, both stats all zero.
 *   - errors: those of SEED SETS, plus a NULL row_ptr and a bad threshold (FORA_E_ARG).  No device memory for the accumulator
 *     block, the rank block or the result: FORA_E_NOMEM, nothing held, the ctx still usable.
 *   - a held sparse result, the walk index, the options and the FORA parameters are left untouched; fora_timing as in SEED SETS.
 * PROPAGATE (fora_hip_sparse_propagate): feature propagation Z = PI * H over the held sparse result of SPARSE RESULTS or SEED
 * SETS, SPARSE -- out[i][c] = sum over the entries e of row i of w_e * H[id_e][c], computed on the GPU.  The order of the
 * operations is fixed, so every output bit is defined (tests/propagate_ref.py is the twin).
 *   - row i is the entries [row_ptr[i], row_ptr[i+1]) of the held result, in held order (ids ascending).  row_ptr (nq + 1
 *     entries, host memory) is the caller's array as the sparse call returned it; it is validated -- row_ptr[0] == 0,
 *     non-decreasing, row_ptr[nq] == the held entries -- and anything else is FORA_E_ARG.
 *   - w_e = ldexp((double)fix_e, -62), the double fora_hip_sparse_fetch writes to vals (u64 -> f64 rounds to nearest even).
 *     h = (double)H[id_e][c]; H is row-major, n rows (the graph's n) of d columns, leading dimension ldf >= d in elements;
 *     feat_type FORA_PROP_F32: IEEE f32, FORA_PROP_BF16: bf16 widened exactly (bits << 16 as f32).  term_e = w_e * h is one
 *     IEEE f64 multiply, never fused with the add that follows.
 *   - segments: a row is cut every FORA_PROP_SEG = 256 entries counted from its first entry.  P_s = the terms of segment s
 *     added one after the other in entry order, starting from +0.0.  acc = P_0, then acc = acc + P_s for s = 1, 2, ... in
 *     order.  A row of at most 256 entries is a plain left-to-right sum; an empty row gives +0.0.
 *   - flag FORA_PROP_NORMALIZE: S = the integer sum of the row's fix words (u64, wrapping; it cannot wrap in practice: at most
 *     2^62 + 2^10 k for seed sets); acc = acc / ldexp((double)S, -62), one IEEE division, skipped when S == 0.
 *   - out64[i*ldo + c] = acc; out32[i*ldo + c] = (float)acc, rounded to nearest even.  Either may be NULL, both NULL is
 *     FORA_E_ARG.  ldo >= d; the columns d .. ldo of an output are not written.
 *   - feat, out32 and out64 may each be pageable host memory or device memory on the ctx's GPU; a device pointer is read or
 *     written by the device, never staged through the host; memory of another GPU is FORA_E_ARG.  A device feat needs only
 *     element alignment: any base offset and any ldf are legal (a column slice of a wider tensor).  A host feat is uploaded
 *     on every call into a buffer the ctx owns, which only grows and is freed by fora_hip_set_graph and fora_hip_destroy;
 *     callers that propagate repeatedly pass device memory.  A host output is staged in nq * d elements of device memory.
 *   - non-finite features follow the IEEE rules; nothing is checked.
 *   - no bit depends on the batch size, on how the work is split across workgroups and lanes, on whether pointers are host or
 *     device, or on the option "prop_segs" (segments whose partial sums are live at a time: a call runs in chunks of that many
 *     segments; 0: by free memory, otherwise at least 1; readable from the environment like the other non-schedule knobs).
 *   - stats: entries, segments = sum over the rows of ceil(len / 256), max_row, feat_bytes = entries * d * element size,
 *     chunks = max(1, ceil(segments / prop_segs)), feat_on_device, and the device times of the two kernels.
 *   - the held sparse result, a held sweep profile, the walk index, the options, the FORA parameters and fora_timing are left
 *     untouched; the call may be repeated with other features.  The ctx's stream is synchronised before it returns.
 *   - NULL ctx: answered without touching the GPU.  No held sparse result, nq < 0, NULL row_ptr, a row_ptr that does not match
 *     the held result, NULL feat with entries to read, d < 1 or d > 65536, ldf < d, ldo < d, an unknown feat_type or flag bit:
 *     FORA_E_ARG, and nothing is written.  No device memory for the upload, the partial sums or a staged output:
 *     FORA_E_NOMEM, nothing written, the ctx still usable and the held result intact.  nq == 0: FORA_OK, nothing is written.
 * PROPAGATE, TRANSPOSED (fora_hip_sparse_propagate_t, fora_hip_sparse_transpose_fetch): out = PI^T * G over the held sparse
 * result, n x d -- with G = dL/dZ the gradient of the loss with respect to the H of PROPAGATE.  Every output bit is defined
 * (tests/propagate_t_ref.py is the twin).
 *   - the transposition: column v (a node, 0 <= v < n) lists the held entries whose id is v by ascending row index i.  A held
 *     row lists a node at most once (duplicate sources are separate rows), so the order is strict and any correct construction
 *     gives the same arrays: col_ptr (n + 1 prefix sums), rows[p] (the row index of entry p), fix[p] (its held word),
 *     vals[p] = ldexp((double)fix[p], -62).  It is a stable counting sort of the held entries by id, made on the GPU.
 *   - fora_hip_sparse_transpose_fetch copies these arrays; every pointer may be NULL, and may be pageable host memory or device
 *     memory of the ctx's GPU.  cap < the held entries, no held result, a row_ptr that is not the held result's: FORA_E_ARG and
 *     nothing is written.
 *   - the product: out[v][c] = sum over column v's entries e, in that order, of w'_e * (double)G[row_e][c].  grad is row-major
 *     nq x d with pitch ldg >= d; grad_type FORA_PROP_F32 or FORA_PROP_BF16 as for feat in PROPAGATE.  Without a flag
 *     w'_e = ldexp((double)fix_e, -62).  With FORA_PROP_NORMALIZE w'_e = ldexp((double)fix_e, -62) / ldexp((double)S_i, -62), one
 *     IEEE division, S_i the integer sum of the words of row i = row_e (u64, wrapping, as in PROPAGATE): the adjoint of the
 *     normalised forward product.  term = w'_e * g is one IEEE f64 multiply, never fused with the add that follows.
 *   - segments of FORA_PROP_SEG = 256 entries are counted from the column's first entry: P_s summed from +0.0 in entry order,
 *     acc = P_0, then acc = acc + P_s for s = 1, 2, ... -- the PROPAGATE rule with "row" read as "column".  Nothing is divided
 *     after the sum.
 *   - all n output rows are written: a node no row keeps gets +0.0.  out64[v*ldo + c] = acc, out32 = (float)acc rounded to
 *     nearest even; either may be NULL, the columns d .. ldo of an output row are left alone.  A row of grad whose held row is
 *     empty is never read by a sum.  Non-finite values follow IEEE; nothing is checked.
 *   - grad, out32 and out64 may each be host or device memory as in PROPAGATE.  A host grad is uploaded on every call,
 *     (nq - 1) * ldg + d elements; a host output is staged in n * d elements.
 *   - no bit depends on the batch size, on host versus device pointers, on the launch shape, on "prop_segs" (which chunks this
 *     product as it chunks the forward one), on which sort tier a column took, or on the option "propt_lds_cap": a column's run
 *     of 2 .. 64 entries is sorted by a wave, one of up to "propt_lds_cap" entries (default and at most 4096) by a workgroup in
 *     LDS, a longer one in device memory; a run longer than the cap goes to device memory whatever its length, so 0 sends
 *     every run of two entries or more there.
 *   - lifetime: the transposition, the row sums S_i and a device copy of col_ptr are built by the first of the two calls after
 *     a sparse result becomes held, kept with it and reused by later calls (built = 0, transpose_ms = 0).  They end with the
 *     held result -- the next fora_hip_query_sparse_batch or fora_hip_seeds_sparse_batch (whatever that call returns),
 *     fora_hip_sparse_clear, fora_hip_set_graph, fora_hip_destroy -- and when "propt_lds_cap" is set to another value (or the
 *     options are reset), which leaves the held result alone.  row_ptr must be the array the sparse call returned, on every call.
 *   - the held result, a held sweep profile, the walk index, the options, the FORA parameters and fora_timing are left
 *     untouched by both calls; fora_hip_sparse_propagate gives the same bits before and after a transposition exists.
 *   - stats: entries, columns = nodes with at least one entry, segments = sum over the columns of ceil(len / 256), max_col,
 *     feat_bytes = entries * d * element size, chunks, feat_on_device, built, and -- when built -- the columns each tier
 *     sorted (a column of one entry is sorted by none); transpose_ms spans the build, the host's prefix sum included.
 *   - errors: the FORA_E_ARG cases of PROPAGATE (no held result, a bad row_ptr, d outside 1 .. 65536, ldg < d, ldo < d, an
 *     unknown type or flag, both outputs NULL, memory of another GPU) and a NULL grad while the held result has entries:
 *     nothing is written.  FORA_E_NOMEM: nothing written, no half-built transposition kept, the held result intact and the
 *     ctx usable.  NULL ctx: answered without touching the GPU.  nq == 0 (an empty held result): FORA_OK, grad may be NULL,
 *     the outputs are all +0.0.
 *   - fora_hip_get_option "sparse_generation" (read-only): a counter that increases every time a sparse result becomes held
 *     or stops being held; a caller that keeps a row_ptr across calls (an autograd function) compares it to know that the
 *     held rows are still the ones it saw.
 * SCORES (SDDMM) (fora_hip_sparse_sddmm): one dot product per held entry -- for entry e, at place e of the held result, in row
 * i with id v, score_e = <a[i], b[v]> over d columns.  The held rows are the sparsity pattern only: no word is read.  It is
 * the attention logit of a model over the held neighbourhoods, and the gradient of PROPAGATE WITH VALUES with respect to the
 * values.  Every output bit is defined (tests/sddmm_ref.py is the twin).
 *   - row_ptr: validated exactly as in PROPAGATE.  a is row-major nq x d on the row side, pitch lda >= d; b is row-major n x d
 *     on the node side, pitch ldb >= d.  a_type and b_type are each FORA_PROP_F32 or FORA_PROP_BF16 (widened exactly), chosen
 *     independently.  d in 1 .. 65536.
 *   - t_c = (double)a[i][c] * (double)b[v][c], one IEEE f64 multiply; it is exact (two significands of 24 bits, and the
 *     exponents fit), so only the adds round and their order is the contract:
 *       q_l, l = 0 .. 63: the t_c with c == l (mod 64), added one after the other in ascending c, starting from +0.0;
 *       then for o = 32, 16, 8, 4, 2, 1 in this order: q_l = q_l + q_{l+o} for every l < o;
 *       score_e = q_0.
 *     No q_l is ever -0.0 (each starts from +0.0), and a q_l with no column is +0.0, so for d <= 32 the first steps of the
 *     tree add +0.0 and change no bit: a narrower lane group that runs only its own steps gives the same result.  No multiply
 *     is fused with an add.  Non-finite values follow IEEE; nothing is checked.
 *   - out64[e] = score_e; out32[e] = (float)score_e, rounded to nearest even.  Either may be NULL, both NULL is FORA_E_ARG.
 *     cap = the entries each non-NULL output can take; cap < the held entries is FORA_E_ARG and nothing is written.
 *   - a, b, out32 and out64 may each be pageable host memory or device memory on the ctx's GPU (memory of another GPU is
 *     FORA_E_ARG).  A device operand needs only element alignment: any base, any pitch, a column slice of a wider tensor.
 *     A host a is uploaded on every call ((nq - 1) * lda + d elements), a host b likewise ((n - 1) * ldb + d elements); a
 *     host output is staged in `entries` elements of device memory.  These buffers are the ctx's, shared with PROPAGATE.
 *   - a row of a whose held row is empty is never read by a product; columns at or past d are never read.
 *   - no bit depends on the batch size, on "prop_segs", on how the work is split across workgroups and lanes, on alignment,
 *     or on host versus device pointers.
 *   - stats: entries, segments and max_row as in PROPAGATE, bytes = entries * d * (a's element size + b's element size),
 *     a_on_device, b_on_device, and the device time of the kernel.
 *   - the held result, its transposition, a held sweep profile, the walk index, the options, the FORA parameters and
 *     fora_timing are left untouched.  The ctx's stream is synchronised before it returns.
 *   - errors: NULL ctx is answered without touching the GPU.  No held result, nq < 0, NULL row_ptr, a row_ptr that does not
 *     match, NULL a or b with entries to read, d outside 1 .. 65536, lda < d, ldb < d, an unknown a_type or b_type, both
 *     outputs NULL, cap too small: FORA_E_ARG, nothing written.  No device memory for an upload or a staged output:
 *     FORA_E_NOMEM, nothing written, the ctx usable and the held result intact.  nq == 0: FORA_OK, nothing is written.
 * ROW SOFTMAX (fora_hip_sparse_softmax, fora_hip_sparse_softmax_bwd): softmax of one score per held entry inside every held
 * row, and its gradient -- between SCORES (SDDMM) and PROPAGATE WITH VALUES the third step of attention over the held
 * neighbourhoods.  The held rows are the pattern only: no word is read.  Every output bit is defined, the exponential
 * included (tests/softmax_ref.py is the twin).
 *   - exp_def(t), for t <= 0 and t = -inf (NaN never reaches it): t < -708.0 or t = -inf gives +0.0, so no result is ever
 *     subnormal.  Otherwise k = rint(t * LOG2E), one multiply and a rounding to nearest even; r = (t - k * LN2_HI) - k * LN2_LO
 *     with LOG2E = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42feep-1 (21 trailing zero bits: k * LN2_HI is exact for
 *     |k| <= 1022) and LN2_LO = 0x1.a39ef35793c76p-33; p = c13, then p = p * r + c_j for j = 12 .. 0, each step one multiply
 *     and one add, never fused, c_j = 1.0 / (double)(j!) (one IEEE division of two exact doubles; 13! < 2^53); the result is
 *     p * two_k, one multiply, two_k the double with biased exponent k + 1023 and zero significand (k in [-1021, 0]).
 *     exp_def(+-0.0) is exactly 1.0.
 *   - forward: scores has one element per held entry, in held order; val_type FORA_PROP_F32 or FORA_PROP_F64, host or device
 *     memory as the values of PROPAGATE WITH VALUES.  scale: a finite double, anything else is FORA_E_ARG.
 *     x_e = (double)scores[e] * scale, one multiply.  m_i = the row's largest x_e.  If an x_e of the row is NaN, or m_i is
 *     +inf, or m_i is -inf (every entry is -inf), all outputs of the row are the quiet NaN 0x7FF8000000000000 (as f32:
 *     0x7FC00000).  Otherwise m_i is finite; whether +0.0 or -0.0 wins a tie changes no bit.  p_e = exp_def(x_e - m_i): an
 *     entry of -inf or one more than 708 below the maximum gives +0.0, the maximum gives exactly 1.0, so S_i >= 1.
 *   - the row sum S_i: the row is cut every FORA_PROP_SEG = 256 entries counted from its first entry.  In a segment q_l,
 *     l = 0 .. 63, is the sum of the p at the segment-relative positions j == l (mod 64), added in ascending j starting from
 *     +0.0; then for o = 32, 16, 8, 4, 2, 1: q_l = q_l + q_{l+o} for every l < o; P_s = q_0.  S = P_0, then S = S + P_s for
 *     s = 1, 2, ... in order -- the lane order of SCORES (SDDMM) inside the segments of PROPAGATE.
 *   - y_e = p_e / S_i, one IEEE division; out64[e] = y_e, out32[e] = (float)y_e rounded to nearest even.  An empty row writes
 *     nothing.  cap, the NULL outputs and host or device pointers as in SCORES (SDDMM).
 *   - backward: y is the forward output as the caller holds it (y_type f32 or f64), grad is g = dL/dy (g_type f32 or f64,
 *     chosen independently), scale the forward call's.  t_e = (double)y_e * (double)g_e, one multiply; D_i = the row's sum
 *     of t_e in exactly the order of S_i; dx_e = ((g_e - D_i) * y_e) * scale -- a subtraction, then two multiplies; outputs
 *     as in the forward call.  Non-finite values follow IEEE; nothing is checked.  scale is a number, not a differentiable
 *     operand: a learned temperature multiplies the scores before the call.
 *   - both calls: row_ptr is validated as in PROPAGATE.  No bit depends on the batch size, on the launch shape, on host
 *     versus device pointers, on "prop_segs", or on the option "softmax_short": a row of at most that many entries (default
 *     and at most 256) is read once and written once by one wave; a longer one goes segment by segment through partial
 *     maxima and sums; 0 sends every row there.  The option is readable from the environment like the other non-schedule
 *     knobs.
 *   - stats: entries, segments and max_row as in PROPAGATE; nan_rows = the forward rows written as NaN (0 in the backward
 *     call); short_rows and long_rows = the non-empty rows per path; in_on_device (scores, or y), grad_on_device; softmax_ms
 *     = the device time of the call's kernels.
 *   - the held result, its transposition, a held sweep profile, the walk index, the options, the FORA parameters and
 *     fora_timing are left untouched.  The ctx's stream is synchronised before it returns.
 *   - errors: NULL ctx is answered without touching the GPU.  No held result, nq < 0, NULL row_ptr, a row_ptr that does not
 *     match, a NULL input with entries to read, an element type other than the two, a scale that is not finite, both outputs
 *     NULL, cap too small, memory of another GPU: FORA_E_ARG, nothing written.  No device memory for an upload, the
 *     partials or a staged output: FORA_E_NOMEM, nothing written, the ctx usable and the held result intact.  nq == 0:
 *     FORA_OK, nothing is written.
 * ATTENTION (fora_hip_sparse_attention): SCORES (SDDMM), ROW SOFTMAX and PROPAGATE WITH VALUES over the held rows in one call,
 * for `heads` column slices at once -- out = softmax_row(scale * <q, k>) * v on the held pattern.  Every output bit is
 * defined as the composition of those three contracts (tests/attention_ref.py is the twin).
 *   - q is row-major nq x heads * d on the row side, pitch ldq; k is n x heads * d and v is n x heads * dv on the node side,
 *     pitches ldk and ldv; out is nq x heads * dv, pitch ldo.  q_type, k_type and v_type are each FORA_PROP_F32 or
 *     FORA_PROP_BF16 (widened exactly), chosen independently.  d and dv in 1 .. 65536, heads >= 1 with heads * d and
 *     heads * dv at most 65536; ldq, ldk >= heads * d; ldv, ldo >= heads * dv; scale a finite double.
 *   - per head j, with A = q[:, j*d : (j+1)*d], B = k[:, j*d : (j+1)*d] and H = v[:, j*dv : (j+1)*dv]:
 *       score_e is exactly SCORES (SDDMM) of (A, B): the 64 lane sums and the tree, in f64;
 *       y_e is exactly ROW SOFTMAX of those f64 scores with `scale`: exp_def, the row sum in the 64-lane order inside
 *         segments of 256 entries, one division;
 *       out[i][j*dv + c] is exactly PROPAGATE WITH VALUES of H with the f64 y_e as the values: segments of 256 entries added in
 *         entry order from +0.0, acc = P_0, acc = acc + P_s.
 *     Nothing is rounded to f32 between the steps: the call equals fora_hip_sparse_sddmm (out64), fora_hip_sparse_softmax (F64
 *     in, out64) and fora_hip_sparse_propagate_vals (F64 values) on the column slices, bit for bit, in out64 wherever no NaN
 *     row is involved.  out32 = (float)out64, rounded to nearest even.  Either may be NULL, both NULL is FORA_E_ARG.
 *   - y64[j * entries + e] = y_e and y32 = (float)y_e: optional outputs of the probabilities, head by head, which a backward
 *     pass needs.  Both may be NULL.  ycap = the elements each non-NULL one can take; ycap < heads * entries with a non-NULL
 *     y output is FORA_E_ARG.
 *   - a (row, head) whose softmax row is a NaN row by the rule of ROW SOFTMAX (a NaN score, a maximum of +inf, or all -inf)
 *     is written, not computed: its y entries and its dv outputs are the quiet NaN 0x7FF8000000000000 (as f32: 0x7FC00000),
 *     and it is counted in nan_rows.  The products define no NaN payload, so on such rows the chained calls agree in
 *     NaN-ness only.  An empty row writes +0.0 to its heads * dv outputs and nothing to y.
 *   - q, k, v, out32, out64, y32 and y64 may each be pageable host memory or device memory on the ctx's GPU (memory of another
 *     GPU is FORA_E_ARG).  A device operand needs only element alignment: any base, any pitch, a column slice of a wider
 *     tensor.  A host q is uploaded on every call ((nq - 1) * ldq + heads * d elements), a host k and v likewise
 *     ((n - 1) * pitch + columns elements); host outputs are staged in device memory.  These buffers are the ctx's.
 *   - no bit depends on the batch size, on "prop_segs", on "softmax_short", on host versus device pointers, on the launch
 *     shape, or on the option "attn_short": a non-empty row of at most that many entries (default and at most 256) is one
 *     wave's per head in a fused kernel -- scored, normalised and multiplied without anything leaving the CU; a longer one
 *     goes through the kernels of the three steps inside the same call, one head at a time; 0 sends every row there.  The
 *     option is readable from the environment like the other non-schedule knobs.
 *   - stats: entries, segments and max_row as in PROPAGATE; nan_rows counts (row, head) pairs; short_rows and long_rows = the
 *     non-empty rows per path; q_on_device, k_on_device, v_on_device; attn_ms = the device time of the call's launches.
 *   - the held result, its transposition, a held sweep profile, the walk index, the options, the FORA parameters and
 *     fora_timing are left untouched.  The ctx's stream is synchronised before it returns.
 *   - errors: NULL ctx is answered without touching the GPU.  The FORA_E_ARG cases of SCORES (SDDMM) (no held result, nq < 0,
 *     NULL row_ptr, a row_ptr that does not match, a NULL operand with entries to read, an unknown element type, memory of
 *     another GPU), a scale that is not finite, heads < 1, a width or a pitch out of range, both outs NULL, ycap too small:
 *     nothing written.  FORA_E_NOMEM: nothing written, the ctx usable and the held result intact.  nq == 0: FORA_OK, nothing
 *     is written.
 * ATTENTION, BACKWARD (fora_hip_sparse_attention_bwd): the gradients of ATTENTION with respect to q, k and v, for all heads in
 * one call.  Every output bit is defined as a composition of contracts above (tests/attention_bwd_ref.py is the twin).
 *   - q, k, v, their types and pitches, d, dv, heads and scale are the forward call's.  g = dL/dout is nq x heads * dv,
 *     FORA_PROP_F32 or FORA_PROP_BF16, pitch ldg >= heads * dv.  y is [heads][entries], FORA_PROP_F32 or FORA_PROP_F64: what
 *     the forward call wrote to y32 or y64.  ycap = the elements y holds; ycap < heads * entries is FORA_E_ARG.
 *   - per head j, on the column slices [j*d, (j+1)*d) of q and k and [j*dv, (j+1)*dv) of v and g:
 *       dy_e is exactly SCORES (SDDMM) of (g slice, v slice), in f64;
 *       ds_e is exactly ROW SOFTMAX backward of (y_j, dy) with `scale`: the f64 dy as grad, y in the caller's type, in f64;
 *       dq[i][j*d + c] is exactly PROPAGATE WITH VALUES of the k slice with the f64 ds as the values;
 *       dk[v][j*d + c] is exactly PROPAGATE WITH VALUES, transposed, of the q slice with the f64 ds as the values;
 *       dv[v][j*dv + c] is exactly PROPAGATE WITH VALUES, transposed, of the g slice with y_j, in the caller's type, as the
 *         values.
 *     Nothing is rounded to f32 between the steps: in every f64 output the call equals fora_hip_sparse_sddmm (out64),
 *     fora_hip_sparse_softmax_bwd (F64 grad, out64), fora_hip_sparse_propagate_vals (F64 values) and
 *     fora_hip_sparse_propagate_t_vals (F64 values) chained on the column slices, bit for bit.  The f32 outputs are (float) of
 *     the f64 outputs, rounded to nearest even.
 *   - non-finite values follow IEEE as in ROW SOFTMAX backward: nothing is checked and no payload is defined.  Where a NaN
 *     is involved the chained calls and the twin agree in NaN-ness only.
 *   - outputs (fora_attn_grads): dq is nq x heads * d, dk is n x heads * d, dv is n x heads * dv; each as f32 and / or f64
 *     with one pitch per gradient (lddq, lddk >= heads * d; lddv >= heads * dv; the pitch of an absent gradient is not
 *     read).  A gradient with both pointers NULL is absent and costs nothing: with dq and dk both absent dy and ds are never
 *     computed.  All three absent is FORA_E_ARG.  An empty row writes +0.0 to its dq; a column with no entry writes +0.0 to
 *     its dk and dv -- all n columns when the held result has no entries and nq > 0.
 *   - q, k, v, g, y and the six outputs may each be pageable host memory or device memory on the ctx's GPU (memory of another
 *     GPU is FORA_E_ARG).  A device operand needs only element alignment: any base, any pitch, a column slice of a wider
 *     tensor.  Host operands are uploaded on every call and host outputs are staged in device memory, as in ATTENTION.
 *   - no bit depends on the batch size, on "prop_segs", on "softmax_short", on "propt_lds_cap", on host versus device
 *     pointers, on the launch shape, on whether the column plan came from the cache, or on the option "attn_short", which
 *     bounds rows and columns alike: a row of at most that many entries is one wave's per head in k_attn_bwd_short (dy, ds
 *     and dq without anything but ds leaving the CU), a non-empty column of at most that many entries is one lane group's
 *     per head in k_attn_cols; the longer rows and the longer columns go through the kernels of the chained calls inside
 *     the same call, one head at a time; 0 sends everything there.
 *   - the transposition of the held result and its places (PROPAGATE WITH VALUES) are built when dk or dv is wanted and they
 *     are missing -- exactly what the first fora_hip_sparse_propagate_t_vals would do; stats.built = 1 then.  The split of
 *     the columns is planned once per transposition, "attn_short" and chunk size, and kept on the device with it: a second
 *     call plans and uploads nothing on the column side and reports plan_cached = 1.
 *   - stats: entries, segments, max_row, short_rows and long_rows as in ATTENTION; columns = the non-empty columns, max_col,
 *     short_cols and long_cols = the non-empty columns per path (0 when neither dk nor dv is wanted); built, plan_cached; the
 *     five *_on_device flags; transpose_ms = the device time of building (0 unless built); attn_ms = the device time of the
 *     call's other launches.
 *   - the held result, "sparse_generation", a held sweep profile, the walk index, the options, the FORA parameters and
 *     fora_timing are left untouched.  The ctx's stream is synchronised before it returns.
 *   - errors: NULL ctx is answered without touching the GPU.  The FORA_E_ARG cases of ATTENTION, and: a NULL g or y with
 *     entries to read, a y_type other than f32 or f64, a g_type other than f32 or bf16, ycap below heads * entries, a pitch
 *     below its width, all three gradients absent: nothing written.  FORA_E_NOMEM: nothing written, the ctx usable and the
 *     held result intact.  nq == 0: FORA_OK, nothing is written.
 * PROPAGATE WITH VALUES (fora_hip_sparse_propagate_vals, fora_hip_sparse_propagate_t_vals): the products of PROPAGATE and
 * PROPAGATE, TRANSPOSED with the caller's values in place of the held words -- out = P(values) * H and out = P(values)^T * G,
 * P(values) the held pattern with values[e] at held entry e.  Each is the other's gradient with respect to the dense operand,
 * and SCORES (SDDMM) is their gradient with respect to values (tests/propagate_values_ref.py is the twin).
 *   - values: one element per held entry, in held order; val_type FORA_PROP_F32 (widened exactly) or FORA_PROP_F64 (legal for
 *     values only).  w_e = (double)values[e].  Host or device memory; a host array is uploaded on every call.  NULL values
 *     while the held result has entries: FORA_E_ARG.  A val_type other than these two: FORA_E_ARG.
 *   - everything else is the contract of PROPAGATE and of PROPAGATE, TRANSPOSED word for word with w_e read for the weight:
 *     term = w_e * h, one f64 multiply never fused; segments of FORA_PROP_SEG = 256 entries of a row (of a column of the
 *     transposition), P_s from +0.0 in entry order, acc = P_0, acc = acc + P_s; the outputs, the pitches, "prop_segs", the
 *     sort tiers, the stats, what is left untouched, the errors.  In the transposed product entry p of a column takes
 *     values[pos[p]], pos[p] the place of that entry in the held result.
 *   - FORA_PROP_NORMALIZE together with values is FORA_E_ARG: a softmax or a division is the caller's.
 *   - pos belongs to the transposition: it is made by the first call with values after the transposition exists (or with it,
 *     when that call builds it: built = 1) and ends with it.  A call with values on a held result whose transposition
 *     exists reports built = 0 and rebuilds nothing.  The plain calls never make pos, allocate what they always allocated
 *     and give the bits they always gave, before and after a call with values.
 *   - with values equal to the f64 vals of fora_hip_sparse_fetch both calls give the bits of the plain calls without
 *     FORA_PROP_NORMALIZE.
 * NARROW OPERANDS (FORA_PROP_F16, FORA_PROP_E4M3, FORA_PROP_E5M2): three more element types for the dense operands, legal in
 * every argument where FORA_PROP_BF16 is -- feat_type and grad_type of PROPAGATE, of PROPAGATE, TRANSPOSED and of their forms
 * WITH VALUES; a_type and b_type of SCORES (SDDMM); q_type, k_type and v_type of ATTENTION and of ATTENTION, BACKWARD, and its
 * g_type -- each chosen independently of the others.  They stay FORA_E_ARG wherever FORA_PROP_BF16 is: as val_type, as the
 * score, y or grad type of ROW SOFTMAX, as y_type.  The value 3 is no type and FORA_E_ARG everywhere.
 *   - FORA_PROP_F16 is IEEE binary16 with s, e (5 bits), m (10 bits): e = 0 is (-1)^s * m * 2^-24; 1 <= e <= 30 is
 *     (-1)^s * (1024 + m) * 2^(e - 25); e = 31 with m = 0 is +-inf, with m != 0 NaN.
 *   - FORA_PROP_E5M2 is the binary16 whose bits are byte << 8 (torch.float8_e5m2).
 *   - FORA_PROP_E4M3 is the OCP "fn" form (torch.float8_e4m3fn) with s, e (4 bits), m (3 bits): e = 0 is (-1)^s * m * 2^-9,
 *     otherwise (-1)^s * (8 + m) * 2^(e - 10); 0x7F and 0xFF are NaN, there are no infinities, the largest value is 448.
 *   - every value is exactly an f32; -0 stays -0; a NaN code widens to some quiet NaN, and no payload is defined.
 *   - with an operand of a narrow type every call gives, bit for bit and in every output (out32, out64, y32, y64, dq, dk, dv),
 *     what it gives with that operand widened to FORA_PROP_F32 by this rule; where a NaN is involved, NaN-ness is what agrees.
 *     "t_c is exact" of SCORES (SDDMM) keeps holding: the significands only get shorter.
 *   - an operand needs only element alignment -- any byte offset for FP8, any pitch, a column slice of a wider tensor; a host
 *     operand is uploaded by its element size; feat_bytes (fora_prop_stats, fora_propt_stats) and bytes (fora_sddmm_stats)
 *     count 1 or 2 bytes per element.  No option and no launch shape changes a bit.
 * ROW STORE (fora_hip_store_put, fora_hip_store_load, fora_hip_store_take, fora_hip_store_info, fora_hip_store_clear): a library
 * of sparse rows kept on the device, any list of which becomes the held sparse result with one copy on the GPU and no query --
 * the rows of the training nodes are computed once and every mini-batch takes its own.
 *   - the store: one per ctx, rows 0 .. R - 1 as (row_ptr, ids, fix), ids and fix in device memory the ctx owns, outside the
 *     workspace and apart from the held sparse result; row_ptr is kept on the host, where a take is planned.  It lives until
 *     fora_hip_store_clear, fora_hip_set_graph or fora_hip_destroy; every other entry point leaves it untouched -- the sparse
 *     calls that replace the held result, fora_hip_sparse_clear, set_option (a reset too), set_batch, a bucket retry.
 *   - fora_hip_store_put copies the held sparse result into the store, device to device.  row_ptr is validated exactly as in
 *     PROPAGATE.  append == 0 replaces the store; append != 0 adds the nq rows behind the R rows that are there: row i of the
 *     call becomes store row R + i (an append to an empty or absent store fills it).  The held result, its transposition,
 *     "sparse_generation" and everything else stay untouched.  nq == 0 is legal: it adds nothing (and, replacing, leaves an
 *     empty store).  No held result, or a row_ptr that does not match it: FORA_E_ARG, the store unchanged.
 *   - fora_hip_store_load does the same with the caller's arrays: rows fetched earlier, or read from disk, come back.  row_ptr
 *     is a host array of nrows + 1 entries with row_ptr[0] == 0, non-decreasing; row_ptr[nrows] is the number of entries.  ids
 *     and fix may each be pageable host memory or device memory on the ctx's GPU (memory of another GPU is FORA_E_ARG); a device
 *     array is read by the device and never staged through the host, at any element alignment (a slice of a larger tensor).
 *     Every consumer of the held result relies on ids in [0, n) that ascend strictly inside a row, so EVERY entry is checked for
 *     that on the GPU (k_store_check), and the check has finished before anything moves into the store; the smallest offending
 *     entry is named by fora_hip_last_error.  Equal or descending ids across a row boundary are legal.  Words may be any u64.
 *     A bad array or row_ptr, NULL ids or fix while there are entries, nrows < 0, no graph: FORA_E_ARG, the store exactly as it
 *     was.  nrows == 0 with append == 0 leaves an empty store.
 *   - both: no device memory is FORA_E_NOMEM, the store unchanged and the ctx usable.  A call that replaces the store, or an
 *     append that outgrows the room behind the store's entries, builds new arrays and moves them in after its last step; until
 *     then the old store and the new arrays exist side by side.
 *   - fora_hip_store_take makes the rows rows[0 .. nb) of the store the held sparse result, in the caller's order; duplicate
 *     indices give duplicate rows.  Like every call that makes a held result it first ends the one that is held, whatever
 *     becomes of the call, and "sparse_generation" moves as it does for the query calls; the arguments are checked behind that
 *     point, as a bad k is in SPARSE RESULTS, TOP-K.  Held row i has the ids and the words of store row rows[i], in that row's
 *     order, word for word; row_ptr_out (nb + 1) is the prefix sum of the lengths; fora_hip_sparse_fetch gives
 *     vals[e] == ldexp((double)fix[e], -62) as always.  The store is not changed, and the result is an ordinary held result in
 *     every respect: fetch, both products, the transposition, SCORES, ROW SOFTMAX, ATTENTION and its backward pass work on it
 *     unchanged.  nb == 0: FORA_OK, row_ptr_out[0] = 0, an empty result held.  NULL row_ptr_out, nb < 0, NULL rows with nb > 0,
 *     an index outside [0, R) -- against an empty or absent store too: FORA_E_ARG, nothing held.  No device memory:
 *     FORA_E_NOMEM, nothing held, the store intact, the ctx usable.  rows is a host array: row_ptr_out has to reach the host
 *     anyway, every consumer validating the caller's host row_ptr.
 *   - fora_hip_store_info reports R, the store's entries and its longest row; any pointer may be NULL; an empty or absent store
 *     reports zeros.  fora_hip_store_clear frees the store.
 *   - no bit depends on the option "take_span" (the output entries one workgroup of k_store_take copies, and of k_store_check
 *     checks: a multiple of 64 and at least 64, other values are rounded down to one and clamped to 64 .. 65536; readable from
 *     the environment like the other non-schedule knobs), on the launch shape, on host versus device pointers, or on whether
 *     the store was filled by put or by load, at once or by appends.
 *   - stats (fora_store_stats): rows, entries and max_row of this call; store_rows and store_entries of the store after it (a
 *     take: unchanged); ids_on_device and fix_on_device (load); store_ms = the device time of the call's kernel and of the copies
 *     of the call's own rows (the move of the rows that stay, when an append outgrows its room, is not in it).
 *   - a NULL ctx is answered without touching the GPU (FORA_E_ARG).  A held sweep profile, the walk index, the options, the
 *     FORA parameters and fora_timing are left untouched by all five; the ctx's stream is idle when they return.
 * COLUMNS (fora_hip_sparse_compact, fora_hip_sparse_cols_fetch): the held sparse result re-expressed over its own columns -- the
 * node set of a mini-batch.  1000 top-64 rows touch at most 64 000 of a graph's n nodes; after a compaction every call on the
 * held rows has nc columns instead of n, nc the number of distinct ids among the held entries.
 *   - fora_hip_sparse_compact works on whatever sparse result is held (plain, top-k, seed sets, taken from the store); row_ptr
 *     is validated exactly as in PROPAGATE.  U is the set of the distinct ids among the held entries in ascending order; it is
 *     kept on the device.  Every held id is replaced in place by its rank in U, a number in [0, nc) with nc = |U|; the words
 *     and row_ptr are untouched.  The relabelling is monotone: ids still ascend strictly inside a row, and every contract
 *     above holds on the compacted result with nc in the place of n.  *ncols_out = nc (required).
 *   - from then on, and for as long as that result is held, EVERY call on the held rows uses nc where it uses n: feat of
 *     PROPAGATE, b of SCORES, k and v of ATTENTION have nc rows; the output of PROPAGATE, TRANSPOSED and dk / dv of ATTENTION,
 *     BACKWARD have nc rows, and nothing wider is read, cleared or written; the transposition has nc columns and
 *     fora_hip_sparse_transpose_fetch writes nc + 1 entries of col_ptr, none of its columns empty.  With operand rows
 *     X_loc[j] = X[U[j]] every call gives, bit for bit, what it gives on the uncompacted result with X; the outputs over columns
 *     are the uncompacted ones' rows U (whose other rows are +0.0).  fora_hip_sparse_fetch returns the local ids.
 *   - a compaction drops the transposition (it was over n columns) and moves "sparse_generation": the ids changed, and a
 *     backward pass must not run on rows other than its forward pass saw.  fora_hip_get_option("sparse_cols") reads nc while
 *     a compacted result is held and n otherwise.
 *   - the compacted state ends wherever the held result ends: every call that makes a new held result (fora_hip_store_take
 *     included), fora_hip_sparse_clear, fora_hip_set_graph.  The next result is over the n nodes again.
 *   - zero held entries: FORA_OK, nc = 0, U empty.  A result that is compacted already, a NULL ncols_out, no held result or a
 *     row_ptr that is not its own: FORA_E_ARG, nothing changed.  No device memory: FORA_E_NOMEM, nothing changed.  A device
 *     failure behind the first launch leaves nothing held.
 *   - fora_hip_sparse_cols_fetch copies U out: nc int32 node ids, ascending, to pageable host memory or to device memory on the
 *     ctx's GPU (memory of another GPU is FORA_E_ARG).  No compacted result held, or cap < nc: FORA_E_ARG.
 *   - fora_hip_store_put of a compacted result is FORA_E_ARG, the store unchanged: the store holds node ids.
 *   - no bit depends on the option "cols_block" (the bitmap words one workgroup counts: a power of two from 1 to 4096, other
 *     values are clamped and rounded down to one; readable from the environment like the other non-schedule knobs), on the
 *     launch shape, or on the order in which the device meets the entries: the bitmap is written with OR alone.
 *   - stats (fora_cols_stats): entries = the held entries; cols = nc; words = the bitmap words scanned, ceil(n / 64) (0 without
 *     entries); cols_ms = the device time of the bitmap's clear and of the call's kernels.
 *   - a NULL ctx is answered without touching the GPU (FORA_E_ARG).  The store, a held sweep profile, the walk index, the
 *     options, the FORA parameters and fora_timing are left untouched; the ctx's stream is idle when both return.
 */
#ifndef FORA_HIP_H
#define FORA_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FORA_FIX_ONE (1ULL << 62)
#define FORA_STREAM_INDEX 0xFFFFFFFFu
#define FORA_BWD_FIX_ONE (1ULL << 60)

enum {
    FORA_OK = 0,
    FORA_E_ARG = -1,      /* bad argument / call order (reference: assert, graph.h:155) */
    FORA_E_HIP = -2,      /* HIP runtime error, see fora_hip_last_error */
    FORA_E_NOMEM = -3,    /* device memory */
    FORA_E_OVERFLOW = -4, /* internal work list overflow / level cap reached */
    FORA_E_NOGPU = -5     /* no usable gfx950 device */
};

typedef struct fora_ctx fora_ctx;

/* Per-query counters.  Replaces the globals fora_query_basic updates:
 * num_total_rw / num_hit_idx (algo.h:39-40), rsum (query.h:843), plus schedule
 * counters of the level-synchronous push. */
typedef struct {
    double rsum;         /* residue mass left by the push, = rsum_fix * 2^-62 (query.h:843,886) */
    uint64_t rsum_fix;
    uint64_t n_rw;       /* N = (u64)(omega*rsum') of query.h:270 */
    uint64_t n_walks;    /* sum of num_s_rw, query.h:287,318 (num_total_rw) */
    uint64_t n_idx_hit;  /* walks served from the index, query.h:295,306 (num_hit_idx) */
    uint64_t pops;       /* frontier pops of the push */
    uint64_t relax;      /* edge relaxations of the push */
    uint64_t ppr_sum_fix; /* sum of the final ppr vector (== FORA_FIX_ONE when mass is conserved) */
    int32_t levels;      /* push levels this query was active in */
    int32_t dangling_source; /* 1: algo.h:961-965 fast path taken */
    double rmax_used;    /* rmax of the last push round (config.rmax unless --balanced, query.h:877) */
    int32_t push_rounds; /* 1 unless --balanced */
    int32_t reserved_;
} fora_query_stats;

/* Accumulated device timings since the last reset (HIP events on the ctx stream). */
typedef struct {
    double push_pop_ms;     /* sum over k_push_pop launches (direct path only) */
    double push_expand_ms;  /* sum over k_pushq_bin launches (k_push_expand on the direct path) */
    double push_accum_ms;   /* sum over k_accum<false> launches (bucketed push only) */
    double walk_alloc_ms;   /* k_walk_alloc */
    double walk_ms;         /* k_walk_idx + k_walk_online */
    double walk_accum_ms;   /* k_accum<to ppr> (bucketed path only) */
    double other_ms;        /* init / reduce / convert kernels + memsets */
    double batch_ms;        /* whole batches, first launch to last completion */
    uint64_t push_pop_launches;
    uint64_t push_expand_launches;
    uint64_t push_accum_launches;
    uint64_t walk_launches;
    uint64_t batches;
    uint64_t pops;          /* totals over all queries since reset */
    uint64_t relax;
    uint64_t walks;
    uint64_t walk_steps;
    uint64_t levels;        /* levels launched (including speculative empty ones) */
    uint64_t idx_hits;      /* walks served from the index (num_hit_idx, algo.h:39) */
    double push_tail_ms;    /* k_push_tail launches (they finish the push once every frontier is small) */
    uint64_t push_tail_launches;
    double push_team_ms;    /* k_push_team launches (graphs of the narrow layout: the whole push above the tail, one launch per batch) */
    uint64_t push_team_launches;
} fora_timing;

/* Counters of a backward-push sweep (fora_hip_bwdpush_batch, fora_hip_bippr_batch).  Sums over the call's pushes. */
typedef struct {
    uint64_t targets, pops, relax;   /* sums over the call's backward pushes */
    uint64_t entries;                /* non-zero (node, target) reserve + residue entries produced */
    uint64_t global_targets;         /* targets that overflowed the LDS tier */
    int32_t levels, chunks;          /* deepest push; target chunks the call used */
    double bwd_ms, walk_ms, combine_ms;
} fora_bwd_stats;

/* What a sparse call kept (fora_hip_query_sparse_batch). */
typedef struct {
    uint64_t entries;     /* entries kept over the whole call (== row_ptr[nq]) */
    uint64_t max_row;     /* longest row */
    uint64_t thr_fix;     /* the threshold actually applied, in units of 2^-62 */
    int32_t batches;      /* query batches the call ran */
    int32_t reserved_;
    double compact_ms;    /* device time of the compaction kernels, summed over the batches */
} fora_sparse_stats;

/* What a seed-set call ran (fora_hip_query_seeds_batch). */
typedef struct {
    uint64_t seeds;        /* seeds listed over all sets (== set_ptr[ns]) */
    uint64_t distinct;     /* distinct seed ids of the call */
    uint64_t queries;      /* single-source queries actually run (slots taken): distinct non-dangling seeds
                              with dedup on, listed non-dangling seeds with it off */
    uint64_t dangling;     /* listed seeds without out-edges (never take a slot) */
    int32_t batches, reserved_;
    double combine_ms;     /* device time of the combine kernels, summed over the batches */
} fora_seeds_stats;

/* One row of a sweep (fora_hip_sweep_batch): the support's size and the best prefix (0: none). */
typedef struct { int64_t len, best; uint64_t cut, vol, den; double conductance; } fora_sweep_row;
/* What a sweep call ran. */
typedef struct { uint64_t entries, max_row, thr_fix, edges; /* out-edges scanned */
                 int32_t batches, global_rows; /* rows sorted on the global tier */
                 double compact_ms, sort_ms, cut_ms; } fora_sweep_stats;

/* ---- lifecycle ---------------------------------------------------------- */
int fora_hip_device_count(void); /* usable HIP devices (0 when there is none) */
int fora_hip_create(int device, fora_ctx **out);
void fora_hip_destroy(fora_ctx *ctx);
const char *fora_hip_last_error(fora_ctx *ctx);
/* device name / arch string of the ctx's GPU, e.g. "gfx950:sramecc+:xnack-" */
int fora_hip_device_info(fora_ctx *ctx, char *arch, int arch_len, int *cus, uint64_t *hbm_bytes);

/* ---- graph: replaces Graph::init_graph's in-memory result (graph.h:89-163) --
 * CSR with per-row file order; m_attr is the m of attribute.txt (graph.h:58-63),
 * which the parameter formulas use even when it differs from nnz. */
int fora_hip_set_graph(fora_ctx *ctx, int32_t n, int64_t m_attr, const int64_t *row_ptr,
                       const int32_t *col);

/* ---- parameters: replaces init_parameter (graph.h:173-183) + fora_setting
 * (algo.h:455-463); alpha is config.alpha (config.h:27,132). */
int fora_hip_set_params(fora_ctx *ctx, double alpha, double epsilon, double rmax_scale, int opt,
                        uint64_t seed);
/* same, with rmax / omega given directly (tests, --balanced style callers) */
int fora_hip_set_params_raw(fora_ctx *ctx, double alpha, double rmax, double omega, int opt,
                            uint64_t seed);
int fora_hip_get_params(fora_ctx *ctx, double *rmax, double *omega);
/* --balanced (config.balanced; fora_query_basic query.h:848-884, estimated_random_walk_cost :825-838): rmax is
 * halved from 8*rmax while the estimated walk cost omega*rsum*(1-alpha)*t exceeds what the push has cost so far.
 * The reference measures the push with a wall clock (not reproducible); here it is charged by its work counters,
 * pops*c_pop + relax*c_edge seconds, and t = t_walk (t_idx with an index once rmax < config.rmax).  A cost <= 0
 * selects the value calibrated on MI355X (2.0e-11, 2.4e-11, 6.5e-11, 2.2e-11 s: twice the bulk push rate, because
 * the deeper rounds are long cascades of small levels; the reference's constants are
 * t_walk = 4e-7, t_idx = t_walk/140, query.h:822-823).  start_scale: first rmax = start_scale * config.rmax
 * (<= 0: the reference's 8, query.h:862; every round is a whole cascade of levels on the GPU, so callers after
 * throughput start at 1). */
int fora_hip_set_balanced(fora_ctx *ctx, int on, double start_scale, double c_pop, double c_edge, double t_walk,
                          double t_idx);
/* queries processed concurrently per launch; 0 = choose from free HBM */
int fora_hip_set_batch(fora_ctx *ctx, int batch);
int fora_hip_get_batch(fora_ctx *ctx);
/* Engine knobs (layout choice, launch shapes, capacities; the list is `OPTIONS` in fora_hip.hip).  A knob is read
 * once, in fora_hip_create, from the environment variable FORA_HIP_<NAME>; this call changes one afterwards (tests
 * use it to force the wide layout, tiny buckets, the k_push_tail or k_push_team path ...).  None of the knobs the
 * environment can set changes a result bit.  Four knobs choose another push SCHEDULE and with it other (equally valid)
 * residue / reserve / ppr bits: "rounds", "round_div" (threshold rounds), "defer" and "defer_min" (bounded deferral).
 * They are off by default, are NOT read from the environment -- only this call sets them -- and a run with them equals
 * oracle/fora_twin.c run with the same values (orc_twin_set_rounds / _round_div / _defer / _defer_min).
 * name "reset": back to the defaults / the environment values fora_hip_create read.  Unknown name: FORA_E_ARG. */
int fora_hip_set_option(fora_ctx *ctx, const char *name, int64_t value);
/* Reads a knob back, or one of the engine's read-only state words: "team_members" (members per team of k_push_team; 0:
 * this graph / workspace pushes with the bucketed kernels), "team_local_ids" and "team_hub_sums" (local ids and hub sums per
 * member in the team tables built for this graph; both 0 without a team push), "team_cooperative" (1: k_push_team is launched with
 * hipLaunchCooperativeKernel -- option team_coop, off by default), "team_fallbacks" (calls that were run again through the bucketed push because a team of
 * k_push_team timed out waiting for a member -- its workgroups were not co-resident, e.g. another context's kernels held
 * CUs; the caller sees FORA_OK and the same result bits), "team_suspended" (calls left that do not try the team push
 * after such a time-out), "bucket_retries" (calls that were run again with doubled message buckets), "walk_dg_wgs_per_cu"
 * (workgroups of k_walk_dg that one CU holds at this graph's tables, from hipOccupancyMaxActiveBlocksPerMultiprocessor; 0: the
 * graph has no degree-grouped copy), "test_paths" (1: the build with the schedule experiments compiled in, libfora_hip_test.so). */
int fora_hip_get_option(fora_ctx *ctx, const char *name, int64_t *value);

/* ---- walk index: replaces build() (build.h:302-366), rw_idx / rw_idx_info
 * (algo.h:42-43) and deserialize_idx() (build.h:194-207) ------------------- */
int fora_hip_index_sizes(fora_ctx *ctx, uint64_t *total, uint64_t *off /*n or NULL*/,
                         uint64_t *cnt /*n or NULL*/);
int fora_hip_build_index(fora_ctx *ctx); /* walks on the GPU, index stays in HBM */
int fora_hip_get_index(fora_ctx *ctx, int32_t *rw_idx, uint64_t len, uint64_t *off, uint64_t *cnt);
int fora_hip_set_index(fora_ctx *ctx, const int32_t *rw_idx, uint64_t len, const uint64_t *off,
                       const uint64_t *cnt);
int fora_hip_clear_index(fora_ctx *ctx);

/* ---- SSPPR: replaces the query() loop over fora_query_basic
 * (query.h:1471-1476 -> query.h:841-907).  ppr_out: nq*n doubles or NULL
 * (results then stay in HBM; only stats come back).  with_idx: config.with_rw_idx. */
int fora_hip_query_batch(fora_ctx *ctx, const int32_t *sources, int nq, int with_idx,
                         double *ppr_out, fora_query_stats *stats /*nq or NULL*/);
/* same run, raw fixed-point outputs for bit-exact checks (either may be NULL) */
int fora_hip_query_batch_fix(fora_ctx *ctx, const int32_t *sources, int nq, int with_idx,
                             uint64_t *ppr_fix_out, uint64_t *residue_fix_out,
                             fora_query_stats *stats);

/* ---- SSPPR, result kept sparse (the SPARSE RESULTS contract above; the reference keeps ppr sparse too: an iMap with
 * an occur list, algo.h).  fora_hip_query_batch with the rows thresholded and compacted on the GPU into a CSR the ctx
 * holds.  row_ptr: nq + 1 entries, required. */
int fora_hip_query_sparse_batch(fora_ctx *ctx, const int32_t *sources, int nq, int with_idx,
                                double threshold, int64_t *row_ptr,
                                fora_query_stats *stats /*nq or NULL*/, fora_sparse_stats *sp /*or NULL*/);
/* copies the held result; any of ids / vals / fix may be NULL; cap = entries each non-NULL array can take */
int fora_hip_sparse_fetch(fora_ctx *ctx, int32_t *ids, double *vals, uint64_t *fix, uint64_t cap);
int fora_hip_sparse_clear(fora_ctx *ctx);

/* ---- feature propagation over the held sparse result (the PROPAGATE contract above): out = rows * feat, nq x d, in a fixed
 * order of operations.  feat: n x d elements of feat_type, row-major with pitch ldf; out32 / out64: nq x d with pitch ldo. */
#define FORA_PROP_SEG 256
enum { FORA_PROP_F32 = 0, FORA_PROP_BF16 = 1 };
enum { FORA_PROP_F16 = 4, FORA_PROP_E4M3 = 5, FORA_PROP_E5M2 = 6 }; /* NARROW OPERANDS above: legal where FORA_PROP_BF16 is; 3 is no type */
enum { FORA_PROP_NORMALIZE = 1 };
typedef struct { uint64_t entries, segments, max_row, feat_bytes; /* entries * d * element size */
                 int32_t chunks, feat_on_device; double gather_ms, combine_ms; } fora_prop_stats;
int fora_hip_sparse_propagate(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq,
                              const void *feat, int feat_type, int d, int64_t ldf, int flags,
                              float *out32 /*or NULL*/, double *out64 /*or NULL*/, int64_t ldo,
                              fora_prop_stats *ps /*or NULL*/);

/* ---- the transposed product over the held sparse result (the PROPAGATE, TRANSPOSED contract above): out = rows^T * grad,
 * n x d, in a fixed order of operations -- the backward pass of fora_hip_sparse_propagate.  grad: nq x d elements of
 * grad_type, row-major with pitch ldg; out32 / out64: n x d with pitch ldo. */
typedef struct { uint64_t entries, columns /* nodes with >= 1 entry */, segments, max_col, feat_bytes;
                 int32_t chunks, feat_on_device, built /* 1: this call built the transposition */,
                 short_cols, lds_cols, global_cols;   /* columns sorted on each tier by the build (0 when built == 0) */
                 double transpose_ms, gather_ms, combine_ms; } fora_propt_stats;
int fora_hip_sparse_propagate_t(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq,
                                const void *grad /*nq x d*/, int grad_type, int d, int64_t ldg, int flags,
                                float *out32 /*n x d or NULL*/, double *out64 /*n x d or NULL*/, int64_t ldo,
                                fora_propt_stats *ps /*or NULL*/);
/* ---- the two products with the caller's values as the weights (the PROPAGATE WITH VALUES contract above): values has one
 * element of val_type (FORA_PROP_F32 or FORA_PROP_F64) per held entry, in held order, in host or device memory. */
enum { FORA_PROP_F64 = 2 }; /* a val_type only */
int fora_hip_sparse_propagate_vals(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq,
                                   const void *feat, int feat_type, int d, int64_t ldf, int flags /*0*/,
                                   const void *values /*entries*/, int val_type,
                                   float *out32 /*or NULL*/, double *out64 /*or NULL*/, int64_t ldo,
                                   fora_prop_stats *ps /*or NULL*/);
int fora_hip_sparse_propagate_t_vals(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq,
                                     const void *grad /*nq x d*/, int grad_type, int d, int64_t ldg, int flags /*0*/,
                                     const void *values /*entries*/, int val_type,
                                     float *out32 /*n x d or NULL*/, double *out64 /*n x d or NULL*/, int64_t ldo,
                                     fora_propt_stats *ps /*or NULL*/);

/* ---- scores on the held pattern (the SCORES (SDDMM) contract above): out[e] = <a[row of e], b[id of e]> over d columns, in a
 * fixed order of operations.  a: nq x d elements of a_type with pitch lda; b: n x d elements of b_type with pitch ldb. */
typedef struct { uint64_t entries, segments, max_row, bytes; /* entries * d * (a's element size + b's) */
                 int32_t a_on_device, b_on_device; double sddmm_ms; } fora_sddmm_stats;
int fora_hip_sparse_sddmm(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq,
                          const void *a, int a_type, int64_t lda, const void *b, int b_type, int64_t ldb, int d,
                          float *out32 /*entries or NULL*/, double *out64 /*entries or NULL*/, uint64_t cap,
                          fora_sddmm_stats *stats /*or NULL*/);

/* ---- softmax inside every held row and its gradient (the ROW SOFTMAX contract above): one element per held entry in and out,
 * in held order, every bit defined.  scores / y / grad: FORA_PROP_F32 or FORA_PROP_F64 elements in host or device memory. */
typedef struct { uint64_t entries, segments, max_row, nan_rows /* forward rows written as NaN */,
                 short_rows, long_rows;                 /* non-empty rows per path (the option "softmax_short") */
                 int32_t in_on_device /* scores, or y */, grad_on_device; double softmax_ms; } fora_softmax_stats;
int fora_hip_sparse_softmax(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq,
                            const void *scores /*entries*/, int val_type, double scale,
                            float *out32 /*entries or NULL*/, double *out64 /*entries or NULL*/, uint64_t cap,
                            fora_softmax_stats *stats /*or NULL*/);
int fora_hip_sparse_softmax_bwd(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq,
                                const void *y /*entries*/, int y_type, const void *grad /*entries*/, int g_type, double scale,
                                float *out32 /*entries or NULL*/, double *out64 /*entries or NULL*/, uint64_t cap,
                                fora_softmax_stats *stats /*or NULL*/);

/* ---- attention over the held rows (the ATTENTION contract above): scores, softmax inside every row and the weighted product
 * in one call, `heads` column slices at once, every bit the composition of the three calls above. */
typedef struct { uint64_t entries, segments, max_row, nan_rows /* (row, head) pairs written as NaN */,
                 short_rows, long_rows;                 /* non-empty rows per path (the option "attn_short") */
                 int32_t q_on_device, k_on_device, v_on_device, pad_; double attn_ms; } fora_attn_stats;
int fora_hip_sparse_attention(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq,
                              const void *q, int q_type, int64_t ldq /* nq x heads*d */,
                              const void *k, int k_type, int64_t ldk /* n x heads*d */,
                              const void *v, int v_type, int64_t ldv /* n x heads*dv */,
                              int d, int dv, int heads, double scale,
                              float *out32 /*or NULL*/, double *out64 /*or NULL*/, int64_t ldo /* nq x heads*dv */,
                              float *y32 /*or NULL*/, double *y64 /*or NULL*/, uint64_t ycap /* heads x entries */,
                              fora_attn_stats *stats /*or NULL*/);

/* ---- the gradients of that call (the ATTENTION, BACKWARD contract above): dq, dk and dv for all heads in one call, every bit
 * the composition of the calls above.  A gradient with both pointers NULL is not computed. */
typedef struct { float *dq32; double *dq64; int64_t lddq; /* nq x heads*d */
                 float *dk32; double *dk64; int64_t lddk; /* n x heads*d */
                 float *dv32; double *dv64; int64_t lddv; /* n x heads*dv */ } fora_attn_grads;
typedef struct { uint64_t entries, segments, max_row, short_rows, long_rows; /* the rows, as in fora_attn_stats */
                 uint64_t columns, max_col, short_cols, long_cols;           /* the non-empty columns, and per path */
                 int32_t built, plan_cached;                                 /* the transposition was built / the column plan was there */
                 int32_t q_on_device, k_on_device, v_on_device, g_on_device, y_on_device, pad_;
                 double transpose_ms, attn_ms; } fora_attn_bwd_stats;
int fora_hip_sparse_attention_bwd(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq,
                                  const void *q, int q_type, int64_t ldq /* nq x heads*d */,
                                  const void *k, int k_type, int64_t ldk /* n x heads*d */,
                                  const void *v, int v_type, int64_t ldv /* n x heads*dv */,
                                  const void *g, int g_type, int64_t ldg /* nq x heads*dv */,
                                  const void *y, int y_type, uint64_t ycap /* heads x entries */,
                                  int d, int dv, int heads, double scale,
                                  const fora_attn_grads *grads, fora_attn_bwd_stats *stats /*or NULL*/);

/* copies the transposition of the held result; any of col_ptr / rows / fix / vals may be NULL; cap = entries each of rows /
 * fix / vals can take, col_ptr takes n + 1 */
int fora_hip_sparse_transpose_fetch(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq,
                                    int64_t *col_ptr /*n+1 or NULL*/, int32_t *rows, uint64_t *fix, double *vals, uint64_t cap);

/* ---- the row store (the ROW STORE contract above): sparse rows kept on the device; put copies the held result in, load the
 * caller's arrays, take makes a list of the store's rows the held sparse result. */
typedef struct { uint64_t rows, entries, max_row;      /* of this call */
                 uint64_t store_rows, store_entries;   /* the store after the call */
                 int32_t ids_on_device, fix_on_device; /* fora_hip_store_load: where the caller's arrays were */
                 double store_ms; } fora_store_stats;
int fora_hip_store_put(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq, int append, fora_store_stats *st /*or NULL*/);
int fora_hip_store_load(fora_ctx *ctx, const int64_t *row_ptr /*nrows+1, host*/, int64_t nrows,
                        const int32_t *ids, const uint64_t *fix, int append, fora_store_stats *st /*or NULL*/);
int fora_hip_store_take(fora_ctx *ctx, const int64_t *rows /*nb, host*/, int nb, int64_t *row_ptr_out /*nb+1, required*/,
                        fora_store_stats *st /*or NULL*/);
int fora_hip_store_info(fora_ctx *ctx, int64_t *rows, uint64_t *entries, uint64_t *max_row);
int fora_hip_store_clear(fora_ctx *ctx);

/* ---- the held result over its own columns (the COLUMNS contract above): compact relabels the held ids to ranks in the
 * ascending set U of the distinct ones, cols_fetch copies U out. */
typedef struct { uint64_t entries, cols, words; double cols_ms; } fora_cols_stats;
int fora_hip_sparse_compact(fora_ctx *ctx, const int64_t *row_ptr /*nq+1*/, int nq, int64_t *ncols_out /*required*/,
                            fora_cols_stats *st /*or NULL*/);
int fora_hip_sparse_cols_fetch(fora_ctx *ctx, int32_t *cols /*host or device*/, uint64_t cap);

/* ---- local clustering (the SWEEP CUT contract above): fora_hip_query_batch, then per row the sweep over ppr / degree and
 * its best cut, all on the GPU.  The profile stays with the ctx until fetched or replaced. */
int fora_hip_sweep_batch(fora_ctx *ctx, const int32_t *sources, int nq, int with_idx, double threshold,
                         int64_t max_size, int64_t *row_ptr /*nq+1, required: prefix sums of L*/,
                         fora_sweep_row *rows /*nq or NULL*/, fora_query_stats *stats /*nq or NULL*/,
                         fora_sweep_stats *sw /*or NULL*/);
int fora_hip_sweep_fetch(fora_ctx *ctx, int32_t *ids /*sweep order*/, uint64_t *cut, uint64_t *vol, uint64_t cap);
int fora_hip_sweep_clear(fora_ctx *ctx);

/* ---- SSPPR on seed sets (the SEED SETS contract above; the reference personalises on one node only).  ns sets in CSR form:
 * set_ptr ns + 1 entries, seeds / weights set_ptr[ns] entries (weights NULL: uniform).  Any output may be NULL: ppr_out /
 * ppr_fix_out ns*n, ids / scores ns*k (k == 0: no top-k), row_sum_fix_out ns. */
int fora_hip_query_seeds_batch(fora_ctx *ctx, const int64_t *set_ptr /*ns+1*/, const int32_t *seeds,
                               const double *weights /*set_ptr[ns] or NULL*/, int ns, int with_idx,
                               double *ppr_out /*ns*n or NULL*/, uint64_t *ppr_fix_out /*ns*n or NULL*/,
                               int k, int32_t *ids, double *scores /*ns*k or NULL*/,
                               uint64_t *row_sum_fix_out /*ns or NULL*/, fora_seeds_stats *st /*or NULL*/);

/* ---- seed sets, sparse and swept (the SEED SETS, SPARSE and SEED SETS, SWEPT contracts above): the sets of
 * fora_hip_query_seeds_batch, their rows thresholded after the sum and held as a sparse result (fora_hip_sparse_fetch /
 * _clear), or swept and held as a profile (fora_hip_sweep_fetch / _clear).  Nothing dense leaves the device. */
int fora_hip_seeds_sparse_batch(fora_ctx *ctx, const int64_t *set_ptr /*ns+1*/, const int32_t *seeds,
                                const double *weights /*set_ptr[ns] or NULL*/, int ns, int with_idx, double threshold,
                                int64_t *row_ptr /*ns+1, required*/, uint64_t *row_sum_fix_out /*ns or NULL*/,
                                fora_seeds_stats *st /*or NULL*/, fora_sparse_stats *sp /*or NULL*/);
/* ---- top-k sparse rows (the SPARSE RESULTS, TOP-K contract above): the two sparse calls with every row cut to its k largest
 * entries, held in ascending id order as the held sparse result. */
typedef struct { uint64_t support, max_support, k;           /* sum and max of len over the live rows */
                 int32_t cut_rows /* len > k */, lds_rows, global_rows, chunks;
                 double select_ms; } fora_topk_stats;
int fora_hip_query_sparse_topk_batch(fora_ctx *ctx, const int32_t *sources, int nq, int with_idx,
                                     double threshold, int64_t k, int64_t *row_ptr /*nq+1, required*/,
                                     fora_query_stats *stats /*nq or NULL*/, fora_sparse_stats *sp /*or NULL*/,
                                     fora_topk_stats *tk /*or NULL*/);
int fora_hip_seeds_sparse_topk_batch(fora_ctx *ctx, const int64_t *set_ptr /*ns+1*/, const int32_t *seeds,
                                     const double *weights /*set_ptr[ns] or NULL*/, int ns, int with_idx, double threshold,
                                     int64_t k, int64_t *row_ptr /*ns+1, required*/, uint64_t *row_sum_fix_out /*ns or NULL*/,
                                     fora_seeds_stats *st /*or NULL*/, fora_sparse_stats *sp /*or NULL*/,
                                     fora_topk_stats *tk /*or NULL*/);
int fora_hip_seeds_sweep_batch(fora_ctx *ctx, const int64_t *set_ptr /*ns+1*/, const int32_t *seeds,
                               const double *weights /*set_ptr[ns] or NULL*/, int ns, int with_idx, double threshold,
                               int64_t max_size, int64_t *row_ptr /*ns+1, required: prefix sums of L*/,
                               fora_sweep_row *rows /*ns or NULL*/, fora_seeds_stats *st /*or NULL*/,
                               fora_sweep_stats *sw /*or NULL*/);

/* ---- top-k: replaces the topk() loop over get_topk -> fora_query_topk_new +
 * topk_ppr (query.h:1397-1401, 1139-1156, 972-1045; algo.h:592-610), --opt driver.
 * ids / scores: nq*k, score descending (ties: id ascending), padded with (0, 0.0). */
int fora_hip_topk_batch(fora_ctx *ctx, const int32_t *sources, int nq, int k, double epsilon,
                        double rmax_scale, int with_idx, int32_t *ids, double *scores,
                        int32_t *rounds /*nq or NULL*/);

/* ---- top-k with bounds: get_topk without --opt -> fora_query_topk_with_bound + topk_ppr (query.h:1139-1156,
 * 909-969, 639-750; set_ppr_bounds algo.h:1178-1261; if_stop algo.h:1096-1166).  ppr_decay_alpha: config.h:123
 * (0.77).  With with_idx the index must have been built without --opt.  Outputs as fora_hip_topk_batch. */
int fora_hip_topk_bound_batch(fora_ctx *ctx, const int32_t *sources, int nq, int k, double epsilon,
                              double rmax_scale, double ppr_decay_alpha, int with_idx, int32_t *ids,
                              double *scores, int32_t *rounds /*nq or NULL*/);

/* ---- exact SSPPR: replaces fwd_power_iteration / multi_power_iter under gen_exact_topk
 * (query.h:1192-1238, 1240-1307): max_iter Jacobi iterations (config.max_iter_num, config.h:115 = 100) of
 * "keep alpha of every positive residual, push the rest along the out-edges, dangling mass back to the
 * source", run as the level-synchronous push with the smallest threshold (one 2^-62 unit per out-edge).
 * Any of ppr_out (nq*n doubles), ppr_fix_out (nq*n raw) and ids/scores (nq*k, k >= 1, score descending,
 * ties id ascending, padded with (0, 0.0)) may be NULL. */
int fora_hip_power_iteration_batch(fora_ctx *ctx, const int32_t *sources, int nq, int max_iter,
                                   double *ppr_out, uint64_t *ppr_fix_out, int k, int32_t *ids,
                                   double *scores);

/* ---- baselines of the reference's experiments (query.h:1482-1511; get_topk :1139-1166; batch_topk :1553-1611).
 * Both use the ctx's alpha and seed and leave its FORA parameters (fora_hip_get_params) untouched.  Any output pointer may
 * be NULL; ppr_out / *_fix_out: nq*n, ids / scores: nq*k (k == 0: no top-k; else 1 <= k <= min(1024, n), score
 * descending, ties id ascending, padded with (0, 0.0), as fora_hip_topk_batch).  Bad nq / sources, k or epsilon <= 0:
 * FORA_E_ARG. */
/* --algo montecarlo: montecarlo_query (query.h:16-43), omega = montecarlo_setting (algo.h:477-483)
 * 3*log(2/pfail)/epsilon/epsilon/delta with pfail = delta = 1/n; walks as in the RNG contract above.  Stats: n_walks = W,
 * ppr_sum_fix, dangling_source.  Timing: walk_ms. */
int fora_hip_montecarlo_batch(fora_ctx *ctx, const int32_t *sources, int nq, double epsilon,
                              double *ppr_out, uint64_t *ppr_fix_out, int k, int32_t *ids, double *scores,
                              fora_query_stats *stats);
/* --algo fwdpush: forward_local_update_linear (algo.h:954-1018) at rmax = fwdpush_setting (algo.h:485-496)
 * rmax_scale*delta*epsilon*n/m (delta = 1/n, m = m_attr of fora_hip_set_graph), the same push as fora_hip_push_batch;
 * ppr = the reserve (compute_ppr_with_reserve, query.h:243-253), the residue is dropped: sum(ppr) = 1 - rsum.  Stats:
 * pops, relax, rsum, rmax_used, levels.  Timing: the push fields. */
int fora_hip_fwdpush_batch(fora_ctx *ctx, const int32_t *sources, int nq, double epsilon, double rmax_scale,
                           double *ppr_out, uint64_t *reserve_fix_out, uint64_t *residue_fix_out,
                           int k, int32_t *ids, double *scores, fora_query_stats *stats);

/* --algo bippr: bippr_query / bippr_query_topk (query.h:71-193), estimate as in the BIPPR contract above; ppr_out /
 * ppr_fix_out at 2^-60 / 2^60, top-k scores = estimate * 2^-60.  The n backward pushes run once per call (chunk by chunk
 * when their entries outgrow the budget from free HBM; a call of several batches then runs them once per batch) and
 * are shared by every source of it.  Stats: n_walks = W, rmax_used, dangling_source, ppr_sum_fix; every other field 0.
 * Timing: walks, walk_steps, walk_ms; backward push and combine times only in *bwd (NULL: not wanted).  Options
 * "bwd_lds_cap" (entries per LDS table, 0: every target on the global tier) and "bwd_chunk" (targets per chunk, 0: by
 * memory) change no bit. */
int fora_hip_bippr_batch(fora_ctx *ctx, const int32_t *sources, int nq, double epsilon, double rmax_scale,
                         double *ppr_out, uint64_t *ppr_fix_out, int k, int32_t *ids, double *scores,
                         fora_query_stats *stats, fora_bwd_stats *bwd);

/* BiPPR for chosen (source, target) sets, the TARGETED BIPPR contract above: pi(s, t) for every s of `sources` and every t
 * of `targets`, row-major nq x nt; est_out at 2^-60 / est_fix_out at 2^60, either may be NULL.  The nt backward pushes
 * run once per call and are shared by every source (chunk by chunk, once per batch, when their entries outgrow the budget
 * from free HBM).  Options "tgt_lanes" (combine: 0 lane = slot, 1 lane = entry, -1 by the call's shape) and "tgt_span"
 * (entries per wave, 0: by the chunk's size) change no bit. */
int fora_hip_bippr_targets_batch(fora_ctx *ctx, const int32_t *sources, int nq, const int32_t *targets, int nt,
                                 double epsilon, double rmax_scale, double *est_out, uint64_t *est_fix_out,
                                 fora_query_stats *stats, fora_bwd_stats *bwd);

/* ---- stage hooks (same device code as the paths above, exposed for parity tests) */
/* forward push only (forward_local_update_linear, algo.h:954-1018) */
int fora_hip_push_batch(fora_ctx *ctx, const int32_t *sources, int nq, uint64_t *reserve_fix_out,
                        uint64_t *residue_fix_out, fora_query_stats *stats);
/* reverse_local_update_linear for nt targets at the given rmax (the BACKWARD PUSH contract above): dense nt*n outputs at
 * 2^60, either may be NULL; an approximate single-target PPR, pi(s, t) = reserve[s] + sum_v pi(s, v) * residue[v].  Uses
 * the ctx's alpha, leaves its parameters untouched.  Bad targets, rmax <= 0 or out of the fixed point's range:
 * FORA_E_ARG. */
int fora_hip_bwdpush_batch(fora_ctx *ctx, const int32_t *targets, int nt, double rmax,
                           uint64_t *reserve_fix_out, uint64_t *residue_fix_out, fora_bwd_stats *bwd);
/* walk allocation in the reference's f64 arithmetic (query.h:270,282 / :349,:364):
 * residue: n doubles (<= 0 entries get 0 walks); returns N and num_s_rw[n]. */
int fora_hip_walk_counts(fora_ctx *ctx, const double *residue, double rsum, uint64_t *num_s_rw,
                         uint64_t *n_rw);
/* endpoints of `count` walks under the Philox contract (random_walk /
 * random_walk_no_zero_hop, algo.h:124-166) */
int fora_hip_walks(fora_ctx *ctx, uint32_t stream, uint32_t round, int no_zero_hop,
                   const int32_t *starts, const uint64_t *js, int64_t count, int32_t *dests);

/* ---- measurement ----------------------------------------------------------- */
int fora_hip_reset_timing(fora_ctx *ctx);
int fora_hip_get_timing(fora_ctx *ctx, fora_timing *out);
/* diagnostic builds (-DFORA_STAMPS) only: shader-clock cycles per kernel phase summed over workgroups since the last
 * fora_hip_reset_timing; [0..15] k_pushq_bin, [16..31] k_accum.  All zero in a product build. */
int fora_hip_get_stamps(fora_ctx *ctx, uint64_t *out32);

/* ---- TEST ENTRY POINTS: in libfora_hip_test.so (-DFORA_TEST_PATHS=1) only, never in libfora_hip.so, and so not declared
 * here.  They put chosen inputs in front of the sweep's own host functions and kernels; nothing is computed a second way.
 *
 *   int fora_hip_test_sweep_rows(fora_ctx *ctx, const uint64_t *rows_fix (nq * n words), int nq, double threshold,
 *                                int64_t max_size, int64_t *row_ptr (nq + 1, required), fora_sweep_row *rows (nq or NULL),
 *                                fora_sweep_stats *sw (or NULL));
 *     fora_hip_sweep_batch with the caller's rows in place of a query's: the rows are copied into the ppr slabs batch by batch
 *     (fora_hip_set_batch is honoured) and compacted, sorted and swept as a batch's own rows are.  Every row takes a slot (a
 *     row is words, not a source: none is "dangling").  Leaves a held profile for fora_hip_sweep_fetch.
 *
 *   int fora_hip_test_sweep_scan(fora_ctx *ctx, int64_t *diff_cut (L, in: differences, out: cuts), uint64_t *vol (L, in:
 *                                per position, out: prefix sums), int64_t L, uint64_t nnz, uint64_t *out6);
 *     k_sweep_scan on one row of length L under the denominator min(vol, nnz - vol); out6 = len, best, cut, vol, den, edges of
 *     the row it wrote.  Uses buffers of its own: a held profile is left alone.
 *
 *   int fora_hip_test_sparse_rows(fora_ctx *ctx, const uint64_t *rows_fix (nq * n words), int nq, double threshold,
 *                                 int64_t *row_ptr (nq + 1, required), fora_sparse_stats *sp (or NULL));
 *     fora_hip_query_sparse_batch with the caller's rows in place of a query's: the rows are copied into the ppr slabs batch
 *     by batch (fora_hip_set_batch is honoured) and counted, placed and held by the library's own compaction.  Every row
 *     takes a slot.  Leaves a held sparse result of exactly chosen row lengths for fora_hip_sparse_fetch and
 *     fora_hip_sparse_propagate.
 *
 *   int fora_hip_test_sparse_topk_rows(fora_ctx *ctx, const uint64_t *rows_fix (nq * n words), int nq, double threshold,
 *                                      int64_t k, int64_t *row_ptr (nq + 1, required), fora_sparse_stats *sp (or NULL),
 *                                      fora_topk_stats *tk (or NULL));
 *     fora_hip_test_sparse_rows with the selection of SPARSE RESULTS, TOP-K behind it: the caller's rows are counted, written
 *     into the candidate scratch chunk by chunk and cut to their k largest entries by the library's own kernels.
 *
 *   int fora_hip_test_exp(fora_ctx *ctx, const double *t (n, host), int64_t n, double *out (n, host));
 *     exp_def of ROW SOFTMAX on the device, one point per thread, in buffers of its own: the device's bits of the exponential
 *     apart from any softmax.  Every t is <= 0 or -inf. */

#ifdef __cplusplus
}
#endif
#endif
