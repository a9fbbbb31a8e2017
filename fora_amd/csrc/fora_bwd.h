// fora_bwd.h -- backward push (reverse_local_update_linear, algo.h:703-751) and the BiPPR combine (bippr_query,
// query.h:71-124), gfx950.
//
//   reverse CSR     (graph.h's gr)      -> k_rev_count, k_rev_fill (counting sort of the CSR's edges by target)
//   backward push   algo.h:703-751      -> k_bwd_push<false, *> (LDS tier), k_bwd_push<true, *> (global tier)
//   combine         query.h:91-112      -> k_bippr_combine (+ k_transpose_u64 on either side)
//   targeted combine (a list of targets) -> k_bippr_combine_targets<by slot / by entry>, k_bippr_targets_finish
//
// Fixed point 1.0 = BWD_ONE = 2^60 (include/fora_hip.h, FORA_BWD_FIX_ONE).  A push is level-synchronous: every node
// whose residue is over thr pops at the same moment (phase A: snapshot, zero, keep floor(x * afix / 2^62)), then the
// rest y = x - keep goes along every in-edge u -> v as floor(y / outdeg(u)) (phase B, integer atomics).  Every add is
// an integer add, so neither the tier, the workgroup count nor the order of the atomics changes a bit.
#pragma once
#include "fora_kernels.h"

namespace fora {

constexpr uint64_t BWD_ONE = 1ull << 60;
constexpr int BWD_TAB_BITS = 11;
constexpr uint32_t BWD_TAB = 1u << BWD_TAB_BITS; // LDS table slots: 2048 x 20 B
constexpr uint32_t BWD_CAP_MAX = 1536;           // entries per LDS table at most (75 % load; also the frontier's size)
constexpr uint32_t BWD_CAP_DEFAULT = 1024;       // > the p99.9 support of a ws-sized graph's targets (510)
constexpr uint32_t BWD_EMPTY = 0xFFFFFFFFu;
constexpr int BWD_MAX_LEVELS = 1 << 16;
constexpr uint32_t ERR_BWD_LEVELS = 1u << 20;    // a push ran out of levels, or a write pass met more entries than its count pass (neither can happen)

// stat words: [0] pops, [1] relaxations, [2] non-zero reserve + residue entries, [3] deepest push (levels), [4] spills, [7] error flags
enum { BS_POPS = 0, BS_RELAX, BS_ENTRIES, BS_LEVELS, BS_SPILL, BS_BAD, BS_WORDS = 8 }; // (BS_BAD: 1 + a target whose write pass disagreed)

struct BwdDev {
    const int64_t *rin_ptr; // reverse CSR: in-edges of v are rin[rin_ptr[v] .. rin_ptr[v + 1])
    const int32_t *rin;
    const uint32_t *deg;    // out-degrees of the CSR
    const int32_t *targets; // target node of index i
    const uint32_t *list;   // indices i to run (null: 0 .. nlist - 1)
    uint32_t nlist;
    uint32_t cap;           // LDS tier: entries per table
    uint64_t thr, afix;     // pop iff r > thr; keep = floor(x * afix / 2^62)
    uint32_t *cnt;          // count pass: entries (support nodes) of target i
    uint8_t *spilled;       // count pass writes it (1: the LDS table overflowed), write pass reads it
    uint32_t *spill;        // count pass, LDS tier: indices of the overflowing targets
    unsigned long long *stat;
    const uint64_t *off;    // write pass: first entry of target i
    uint32_t *e_node;       // write pass: entries (node, reserve, residue), target-major
    uint64_t *e_p, *e_r;
    uint64_t *g_r, *g_p, *g_fy; // global tier: dense slabs of n words per workgroup (kept zero between targets)
    uint32_t *g_tag, *g_list, *g_fn;
    uint32_t n;
    uint32_t *err;
};

__device__ __forceinline__ uint64_t mul_shr62(uint64_t a, uint64_t b) { // floor(a * b / 2^62), 128-bit product
    return (__umul64hi(a, b) << 2) | ((a * b) >> 62);
}

// global-tier slab words are read and written by other waves of the workgroup between barriers: L2 (agent scope)
// accesses, never a vector-L1 line that an atomic of another wave has made stale
template <typename T> __device__ __forceinline__ T gld(const T *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T> __device__ __forceinline__ void gst(T *p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// barrier of k_bwd_push.  The global tier hands frontier / list / slab words from wave to wave through HBM: a
// workgroup-scope barrier need not wait for those stores to land, so an agent-scope fence goes first
template <bool GLOBAL> __device__ __forceinline__ void bwd_barrier() {
    if (GLOBAL) __threadfence();
    __syncthreads();
}

// slot of node u in the LDS table (inserted if absent); -1 when the table holds `cap` entries already
__device__ __forceinline__ int bwd_lds_insert(uint32_t *keys, uint32_t *used, uint32_t cap, uint32_t u) {
    uint32_t h = (u * 0x9E3779B1u) >> (32 - BWD_TAB_BITS);
    for (uint32_t p = 0; p < BWD_TAB; p++) {
        uint32_t k = *(volatile uint32_t *)&keys[h];
        if (k == BWD_EMPTY) {
            k = atomicCAS(&keys[h], BWD_EMPTY, u);
            if (k == BWD_EMPTY) return atomicAdd(used, 1u) < cap ? (int)h : -1;
        }
        if (k == u) return (int)h;
        h = (h + 1) & (BWD_TAB - 1);
    }
    return -1;
}

// One workgroup per target (grid-stride over the list).  GLOBAL = false: the target's (node -> r, p) table lives in LDS;
// a target whose support outgrows `cap` is dropped and listed in `spill`.  GLOBAL = true: dense slabs of this
// workgroup in HBM plus a list of the touched nodes; never overflows.  WRITE = false: count pass (entry counts,
// counters, spill list); WRITE = true: the same push again, entries written from off[i] on.
template <bool GLOBAL, bool WRITE>
__global__ void __launch_bounds__(BLOCK) k_bwd_push(BwdDev b) {
    constexpr uint32_t TS = GLOBAL ? 1 : BWD_TAB, FS = GLOBAL ? 1 : BWD_CAP_MAX;
    __shared__ uint32_t s_key[TS];
    __shared__ unsigned long long s_r[TS], s_p[TS];
    __shared__ uint16_t s_fs[FS];
    __shared__ unsigned long long s_fy[FS];
    __shared__ uint32_t s_used, s_fcnt, s_ovf, s_wpos;
    __shared__ unsigned long long s_red[BLOCK / 64][2];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t gbase = GLOBAL ? (uint64_t)blockIdx.x * b.n : 0;
    uint64_t *gr = GLOBAL ? b.g_r + gbase : nullptr, *gp = GLOBAL ? b.g_p + gbase : nullptr, *gfy = GLOBAL ? b.g_fy + gbase : nullptr;
    uint32_t *gtag = GLOBAL ? b.g_tag + gbase : nullptr, *glist = GLOBAL ? b.g_list + gbase : nullptr, *gfn = GLOBAL ? b.g_fn + gbase : nullptr;
    for (uint32_t li = blockIdx.x; li < b.nlist; li += gridDim.x) {
        const uint32_t i = b.list ? b.list[li] : li;
        if (!GLOBAL && WRITE && b.spilled[i]) continue; // (uniform: the global tier writes this one)
        const uint32_t t = (uint32_t)b.targets[i];
        bwd_barrier<GLOBAL>(); // the previous target's last reads of the table are done
        if (!GLOBAL)
            for (uint32_t k = threadIdx.x; k < BWD_TAB; k += BLOCK) { s_key[k] = BWD_EMPTY; s_r[k] = 0; s_p[k] = 0; }
        bwd_barrier<GLOBAL>();
        if (threadIdx.x == 0) {
            s_used = 1; s_ovf = 0; s_wpos = 0;
            if (GLOBAL) { gst(&glist[0], t); gst(&gtag[t], 1u); gst(&gr[t], BWD_ONE); }
            else {
                const uint32_t h = (t * 0x9E3779B1u) >> (32 - BWD_TAB_BITS);
                s_key[h] = t; s_r[h] = BWD_ONE;
            }
        }
        uint64_t pops = 0, relax = 0;
        int levels = 0;
        for (;;) {
            bwd_barrier<GLOBAL>(); // (previous phase B complete)
            if (threadIdx.x == 0) s_fcnt = 0;
            bwd_barrier<GLOBAL>();
            // phase A: every node over the threshold pops at once
            const uint32_t slots = GLOBAL ? s_used : BWD_TAB;
            for (uint32_t k = threadIdx.x; k < slots; k += BLOCK) {
                if (GLOBAL) {
                    const uint32_t v = gld(&glist[k]);
                    const uint64_t x = gld(&gr[v]);
                    if (x > b.thr) {
                        const uint64_t keep = mul_shr62(x, b.afix);
                        gst(&gr[v], (uint64_t)0);
                        gst(&gp[v], gld(&gp[v]) + keep);
                        const uint32_t f = atomicAdd(&s_fcnt, 1u);
                        gst(&gfn[f], v);
                        gst(&gfy[f], x - keep);
                    }
                } else {
                    if (s_key[k] == BWD_EMPTY) continue;
                    const uint64_t x = s_r[k];
                    if (x > b.thr) {
                        const uint64_t keep = mul_shr62(x, b.afix);
                        s_r[k] = 0;
                        s_p[k] += keep;
                        const uint32_t f = atomicAdd(&s_fcnt, 1u); // < used <= cap <= BWD_CAP_MAX
                        s_fs[f] = (uint16_t)k;
                        s_fy[f] = x - keep;
                    }
                }
            }
            bwd_barrier<GLOBAL>();
            const uint32_t fc = s_fcnt;
            if (fc == 0) break;
            if (++levels > BWD_MAX_LEVELS) {
                if (threadIdx.x == 0) atomicOr(b.err, ERR_BWD_LEVELS);
                break;
            }
            pops += fc;
            // phase B: the popped rest along every in-edge, one wave per frontier node
            for (uint32_t f = wid; f < fc; f += BLOCK / 64) {
                uint32_t v;
                uint64_t y;
                if (GLOBAL) { v = gld(&gfn[f]); y = gld(&gfy[f]); }
                else { v = s_key[s_fs[f]]; y = s_fy[f]; }
                const int64_t beg = b.rin_ptr[v], end = b.rin_ptr[v + 1];
                relax += (uint64_t)(end - beg);
                for (int64_t k = beg + lane; k < end; k += 64) {
                    const uint32_t u = (uint32_t)b.rin[k];
                    const uint64_t inc = y / b.deg[u];
                    if (!inc) continue;
                    if (GLOBAL) {
                        if (atomicCAS(&gtag[u], 0u, 1u) == 0u) gst(&glist[atomicAdd(&s_used, 1u)], u);
                        atomicAdd((unsigned long long *)&gr[u], (unsigned long long)inc);
                    } else {
                        if (*(volatile uint32_t *)&s_ovf) break;
                        const int h = bwd_lds_insert(s_key, &s_used, b.cap, u);
                        if (h < 0) { s_ovf = 1; break; }
                        atomicAdd(&s_r[h], (unsigned long long)inc);
                    }
                }
            }
            bwd_barrier<GLOBAL>();
            if (!GLOBAL && s_ovf) break;
        }
        bwd_barrier<GLOBAL>();
        const bool ovf = !GLOBAL && s_ovf;
        const uint32_t used = s_used;
        if (!WRITE) {
            if (ovf) {
                if (threadIdx.x == 0) { b.spill[atomicAdd(&b.stat[BS_SPILL], 1ull)] = i; b.spilled[i] = 1; b.cnt[i] = 0; }
                continue;
            }
            uint64_t nz = 0;
            for (uint32_t k = threadIdx.x; k < (GLOBAL ? used : BWD_TAB); k += BLOCK) {
                if (GLOBAL) {
                    const uint32_t v = gld(&glist[k]);
                    nz += (gld(&gp[v]) != 0) + (gld(&gr[v]) != 0);
                } else if (s_key[k] != BWD_EMPTY) nz += (s_p[k] != 0) + (s_r[k] != 0);
            }
            nz = wave_sum(nz);
            if (lane == 0) { s_red[wid][0] = nz; s_red[wid][1] = relax; } // (every lane of a wave counted the wave's rows)
            bwd_barrier<GLOBAL>();
            if (threadIdx.x == 0) {
                uint64_t a = 0, r = 0;
                for (int w = 0; w < BLOCK / 64; w++) { a += s_red[w][0]; r += s_red[w][1]; }
                b.cnt[i] = used;
                if (GLOBAL) b.spilled[i] = 1;
                atomicAdd(&b.stat[BS_POPS], (unsigned long long)pops);
                atomicAdd(&b.stat[BS_RELAX], (unsigned long long)r);
                atomicAdd(&b.stat[BS_ENTRIES], (unsigned long long)a);
                atomicMax(&b.stat[BS_LEVELS], (unsigned long long)levels);
            }
        } else {
            const uint64_t o = b.off[i], room = b.off[i + 1] - o; // (== used: the count pass ran the same push)
            for (uint32_t k = threadIdx.x; k < (GLOBAL ? used : BWD_TAB); k += BLOCK) {
                uint32_t v;
                uint64_t p, r;
                if (GLOBAL) { v = gld(&glist[k]); p = gld(&gp[v]); r = gld(&gr[v]); }
                else { v = s_key[k]; if (v == BWD_EMPTY) continue; p = s_p[k]; r = s_r[k]; }
                const uint32_t w = atomicAdd(&s_wpos, 1u);
                if (w >= room) { atomicOr(b.err, ERR_BWD_LEVELS); atomicMax(&b.stat[BS_BAD], (unsigned long long)(i + 1)); continue; }
                b.e_node[o + w] = v; b.e_p[o + w] = p; b.e_r[o + w] = r;
            }
        }
        if (GLOBAL) { // leave the slabs zero for the next target
            bwd_barrier<GLOBAL>();
            for (uint32_t k = threadIdx.x; k < used; k += BLOCK) {
                const uint32_t v = gld(&glist[k]);
                gst(&gr[v], (uint64_t)0); gst(&gp[v], (uint64_t)0); gst(&gtag[v], 0u);
            }
        }
    }
}

// reverse CSR, step 1: in-degrees
__global__ void __launch_bounds__(BLOCK) k_rev_count(const int32_t *col, uint64_t nnz, uint32_t *indeg) {
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * BLOCK)
        atomicAdd(&indeg[col[e]], 1u);
}
// step 2 (after the host's scan into cursor = rin_ptr[0 .. n)): every edge u -> v lands in v's range, in any order
__global__ void __launch_bounds__(BLOCK) k_rev_fill(const int64_t *row_ptr, const int32_t *col, int32_t n,
                                                    unsigned long long *cursor, int32_t *rin) {
    const int lane = threadIdx.x & 63;
    const uint64_t w0 = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6, nw = ((uint64_t)gridDim.x * BLOCK) >> 6;
    for (uint64_t u = w0; u < (uint64_t)n; u += nw) { // one wave per row
        const int64_t beg = row_ptr[u], end = row_ptr[u + 1];
        for (int64_t e = beg + lane; e < end; e += 64) rin[atomicAdd(&cursor[col[e]], 1ull)] = (int32_t)u;
    }
}

// out[c][r] = in[r][c] for an R x C matrix of u64; 32 x 32 tiles through LDS, tiles numbered along a 1-D grid
__global__ void __launch_bounds__(BLOCK) k_transpose_u64(const uint64_t *in, uint64_t *out, uint64_t R, uint64_t C) {
    __shared__ uint64_t tile[32][33];
    const uint64_t tc_n = (C + 31) / 32;
    const uint64_t tr = blockIdx.x / tc_n, tc = blockIdx.x % tc_n;
    const uint32_t x = threadIdx.x & 31, y0 = threadIdx.x >> 5; // 8 rows per pass
    for (uint32_t y = y0; y < 32; y += BLOCK / 32) {
        const uint64_t r = tr * 32 + y, c = tc * 32 + x;
        if (r < R && c < C) tile[y][x] = in[r * C + c];
    }
    __syncthreads();
    for (uint32_t y = y0; y < 32; y += BLOCK / 32) {
        const uint64_t c = tc * 32 + y, r = tr * 32 + x;
        if (r < R && c < C) out[c * R + r] = tile[x][y];
    }
}

// BiPPR estimate of the chunk's targets i = t0 .. t0 + nt - 1 for the nb slots of the batch (query.h:91-112):
// ppr_b[i] = p_i[s_b] + sum over i's entries (v, p, r) of floor(c_b[v] * r / 2^62).  One wave per target, lane = slot;
// cT: the walk slabs node-major ([n][nb], 2^-62), so an entry reads nb consecutive words; out: node-major [n][nb], 2^-60.
__global__ void __launch_bounds__(BLOCK) k_bippr_combine(const uint64_t *cT, uint32_t nb, const int32_t *src, const uint64_t *off,
                                                         const uint32_t *e_node, const uint64_t *e_p, const uint64_t *e_r,
                                                         uint32_t t0, uint32_t nt, uint64_t *out) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = (uint32_t)(((uint64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6);
    if (i >= nt) return;
    const uint64_t e0 = off[i], e1 = off[i + 1];
    const uint64_t row = (uint64_t)(t0 + i) * nb;
    for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
        const uint32_t bq = b0 + lane;
        const bool act = bq < nb;
        const uint32_t s = act ? (uint32_t)src[bq] : BWD_EMPTY;
        uint64_t acc = 0;
        for (uint64_t e = e0; e < e1; e++) {
            const uint32_t v = e_node[e];
            const uint64_t r = e_r[e], p = e_p[e];
            if (act) {
                if (r) acc += mul_shr62(cT[(uint64_t)v * nb + bq], r);
                if (v == s) acc += p;
            }
        }
        if (act) out[row + bq] = acc;
    }
}

// ---- targeted BiPPR (fora_hip_bippr_targets_batch): the same estimate for a caller's list of targets.  The work is the
// chunk's ENTRY array, cut into spans of `span` entries, one wave per span: one target with 10^5 entries spreads over
// 10^5 / span waves, and a chunk of small targets fills the device just the same.  A wave finds the target of its first
// entry by a binary search in off, walks on across target boundaries with its sums in registers and adds them to the zeroed
// slot-major block out[slot][nt_all] once per (target segment, slot) -- never once per entry.  The adds are integer adds,
// so neither the span, the lane mapping nor the order of the atomics changes a bit.

// index of the target that holds entry e < off[nt]: the largest i with off[i] <= e (a target without entries holds none)
__device__ __forceinline__ uint32_t bpt_owner(const uint64_t *off, uint32_t nt, uint64_t e) {
    uint32_t lo = 0, hi = nt; // off[lo] <= e < off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint64_t readlane_u64(uint64_t x, int k) { // lane k's x, k wave-uniform
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), k);
    return ((uint64_t)hi << 32) | lo;
}

// BY_SLOT = true: lane = slot (blockIdx.y picks the group of 64 slots), c = the walk slabs node-major ([n][nb]): an entry
// reads nb consecutive words.  The wave loads 64 entries at a time, one per lane, and hands them round with v_readlane.
// BY_SLOT = false: lane = entry, c = the walk slabs as the walks wrote them, slot-major ([nb][n]): every lane gathers its
// own entry's word, slot after slot, and a wave sum closes each (segment, slot).  This is the shape of a call with few
// sources (one source keeps 64 lanes busy instead of one) and of a call with few entries (no transpose of the slabs).
// Chunk-relative off / entries as k_bwd_push<*, true> wrote them; the chunk's targets are columns t0 .. t0 + nt - 1.
template <bool BY_SLOT>
__global__ void __launch_bounds__(BLOCK) k_bippr_combine_targets(const uint64_t *c, uint32_t nb, uint64_t n, const int32_t *src,
                                                                 const uint64_t *off, const uint32_t *e_node, const uint64_t *e_p,
                                                                 const uint64_t *e_r, uint32_t t0, uint32_t nt, uint32_t span,
                                                                 uint64_t nt_all, unsigned long long *out) {
    const int lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * (BLOCK / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t ne = off[nt];
    uint64_t a = w * span;
    if (a >= ne) return;
    const uint64_t b = min(ne, a + span);
    uint32_t i = bpt_owner(off, nt, a);
    uint64_t seg_end = min(b, off[i + 1]);
    if (BY_SLOT) {
        const uint32_t bq = blockIdx.y * 64 + lane;
        const bool act = bq < nb;
        const uint32_t s = act ? (uint32_t)src[bq] : BWD_EMPTY;
        const uint64_t *cq = c + (act ? bq : 0);
        unsigned long long *oq = out + (uint64_t)(act ? bq : 0) * nt_all + t0;
        uint64_t acc = 0;
        for (uint64_t e0 = a; e0 < b; e0 += 64) {
            const uint64_t mine = e0 + lane;
            const bool have = mine < b;
            const uint32_t v = have ? e_node[mine] : 0;
            const uint64_t r = have ? e_r[mine] : 0, p = have ? e_p[mine] : 0;
            const int cnt = (int)min((uint64_t)64, b - e0);
            for (int k = 0; k < cnt;) {
                const uint64_t e = e0 + k;
                if (e == seg_end) { // the next target's segment: hand over this one's sum
                    if (act && acc) atomicAdd(&oq[i], (unsigned long long)acc);
                    acc = 0;
                    do i++; while (off[i + 1] <= e);
                    seg_end = min(b, off[i + 1]);
                }
                if (k + 4 <= cnt && e + 4 <= seg_end) { // four gathers in flight
                    uint32_t vk[4];
                    uint64_t rk[4], pk[4], ck[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        vk[u] = (uint32_t)__builtin_amdgcn_readlane((int)v, k + u);
                        rk[u] = readlane_u64(r, k + u);
                        pk[u] = readlane_u64(p, k + u);
                        ck[u] = act && rk[u] ? cq[(uint64_t)vk[u] * nb] : 0;
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        if (ck[u]) acc += mul_shr62(ck[u], rk[u]);
                        if (vk[u] == s) acc += pk[u];
                    }
                    k += 4;
                } else {
                    const uint32_t vk = (uint32_t)__builtin_amdgcn_readlane((int)v, k);
                    const uint64_t rk = readlane_u64(r, k), pk = readlane_u64(p, k);
                    if (act) {
                        if (rk) acc += mul_shr62(cq[(uint64_t)vk * nb], rk);
                        if (vk == s) acc += pk;
                    }
                    k++;
                }
            }
        }
        if (act && acc) atomicAdd(&oq[i], (unsigned long long)acc);
    } else {
        for (;;) {
            for (uint32_t q = 0; q < nb; q++) {
                const uint32_t s = (uint32_t)src[q];
                const uint64_t *cq = c + (uint64_t)q * n;
                uint64_t acc = 0;
                for (uint64_t e = a + lane; e < seg_end; e += 64) {
                    const uint32_t v = e_node[e];
                    const uint64_t r = e_r[e];
                    if (r) {
                        const uint64_t cw = cq[v];
                        if (cw) acc += mul_shr62(cw, r);
                    }
                    if (v == s) acc += e_p[e];
                }
                acc = wave_sum(acc);
                if (lane == 0 && acc) atomicAdd(&out[(uint64_t)q * nt_all + t0 + i], (unsigned long long)acc);
            }
            a = seg_end;
            if (a >= b) break;
            do i++; while (off[i + 1] <= a);
            seg_end = min(b, off[i + 1]);
        }
    }
}

// end of a batch of the targeted call: the sum of every slot's nt words (u64, wrapping) and, when wanted, the words as f64
// at 2^-60
__global__ void __launch_bounds__(BLOCK) k_bippr_targets_finish(const uint64_t *est, uint64_t nt, double *f64, unsigned long long *row_sum) {
    const uint64_t row = (uint64_t)blockIdx.y * nt;
    uint64_t acc = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < nt; j += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t x = est[row + j];
        acc += x;
        if (f64) f64[row + j] = (double)x * 0x1p-60; // (exact scaling: == ldexp((double)x, -60))
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&row_sum[blockIdx.y], (unsigned long long)acc);
}

} // namespace fora
