// fora_propt.h -- the kernels that transpose the held sparse result for PROPAGATE, TRANSPOSED (fora_hip_sparse_propagate_t; the
// contract is in include/fora_hip.h, the tier split in fora_propt_plan.h).  Column v of the transposition lists the held
// entries whose id is v by ascending row: a stable counting sort of the entries by id.  All of it is integer work.
//   k_propt_count       cnt[id] += 1 per held entry (u32 atomics: the sum does not depend on their order), and S_i, the
//                       wrapping sum of row i's words;
//   (the host turns cnt into col_ptr)
//   k_propt_place       entry j of row i takes the next free slot of its column and leaves the key (i << 32) | j there: the
//                       order inside a column is whatever the atomics made it;
//   k_propt_sort_short  runs of at most 64 keys: a wave per run, every lane ranks its key against the others by shuffles;
//   k_propt_sort_lds    runs of at most PROPT_LDS_MAX keys: a workgroup per run, the network of fora_propt_plan.h in LDS;
//   k_propt_sort_step   longer runs: one step of that network in device memory per launch;
//   k_propt_fill        rows[p] = key >> 32, fix[p] = the held word the key points at;
//   k_propt_pos         (PROPAGATE WITH VALUES, on the first call with values) pos[p] = the held place of transposed entry p:
//                       its column v by a search in col_ptr, then v among the ascending ids of row rows[p].
// Row indices inside a column are distinct, so ascending keys are one order only: the bits are defined from the sort on.
#pragma once
#include "fora_kernels.h" // BLOCK
#include "fora_propt_plan.h"

namespace fora {

constexpr uint64_t PROPT_KEY_NONE = ~0ull; // above every key: a row index is below 2^31

// a workgroup per row (grid-stride): the row's ids counted, its words summed
__global__ void __launch_bounds__(BLOCK) k_propt_count(const int64_t *row_ptr, uint32_t nq, const int32_t *ids, const uint64_t *fix, uint32_t n,
                                                       uint32_t *cnt, unsigned long long *rsum) {
    for (uint32_t i = blockIdx.x; i < nq; i += gridDim.x) {
        const int64_t lo = row_ptr[i], hi = row_ptr[i + 1];
        uint64_t s = 0;
        for (int64_t e = lo + threadIdx.x; e < hi; e += BLOCK) {
            const uint32_t v = (uint32_t)ids[e];
            s += fix[e];
            if (v < n) atomicAdd(&cnt[v], 1u);
        }
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
        if ((threadIdx.x & 63u) == 0 && hi > lo) atomicAdd(&rsum[i], (unsigned long long)s); // (zeroed by the host; an integer sum)
    }
}

__global__ void __launch_bounds__(BLOCK) k_propt_place(const int64_t *row_ptr, uint32_t nq, const int32_t *ids, uint32_t n, const int64_t *col_ptr,
                                                       uint32_t *cursor, uint64_t *key, uint64_t entries) {
    for (uint32_t i = blockIdx.x; i < nq; i += gridDim.x) {
        const int64_t lo = row_ptr[i], hi = row_ptr[i + 1];
        for (int64_t e = lo + threadIdx.x; e < hi; e += BLOCK) {
            const uint32_t v = (uint32_t)ids[e];
            if (v >= n) continue;
            const uint64_t slot = (uint64_t)col_ptr[v] + atomicAdd(&cursor[v], 1u);
            if (slot < entries) key[slot] = ((uint64_t)i << 32) | (uint64_t)(e - lo);
        }
    }
}

// a wave per run of at most PROPT_SHORT keys: lane l holds key l; its rank is the number of smaller keys
__global__ void __launch_bounds__(BLOCK) k_propt_sort_short(const PropTRun *runs, uint32_t nruns, uint64_t *key) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r = (uint64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (r >= nruns) return; // (the whole wave)
    const PropTRun run = runs[r];
    const uint32_t len = min(run.len, PROPT_SHORT);
    const uint64_t mine = lane < len ? key[run.first + lane] : PROPT_KEY_NONE;
    uint32_t rank = 0;
    for (uint32_t o = 0; o < len; o++) rank += __shfl(mine, (int)o) < mine;
    if (lane < len) key[run.first + rank] = mine; // (every lane has read before the first one writes: one wave, program order)
}

// one step of the network by a whole workgroup on keys in LDS, and the barrier behind it
__device__ __forceinline__ void propt_lds_step(uint64_t *s_key, uint32_t len, uint32_t P, uint32_t k, uint32_t j) {
    for (uint32_t p = threadIdx.x; p < (P >> 1); p += BLOCK) {
        const PropTPair pr = propt_pair(p, k, j);
        if (pr.hi < len) {
            const uint64_t a = s_key[pr.lo], b = s_key[pr.hi];
            if (a > b) { s_key[pr.lo] = b; s_key[pr.hi] = a; }
        }
    }
    __syncthreads();
}

// a workgroup per run of at most PROPT_LDS_MAX keys: loaded, every step of the network with a barrier behind it, stored
__global__ void __launch_bounds__(BLOCK) k_propt_sort_lds(const PropTRun *runs, uint64_t *key) {
    __shared__ uint64_t s_key[PROPT_LDS_MAX];
    const PropTRun run = runs[blockIdx.x];
    const uint32_t len = min(run.len, PROPT_LDS_MAX);
    for (uint32_t i = threadIdx.x; i < len; i += BLOCK) s_key[i] = key[run.first + i];
    __syncthreads();
    uint32_t P = 1;
    while (P < len) P <<= 1;
    for (uint32_t k = 2; k <= P; k <<= 1) {
        propt_lds_step(s_key, len, P, k, 0);
        for (uint32_t j = k >> 2; j; j >>= 1) propt_lds_step(s_key, len, P, k, j);
    }
    for (uint32_t i = threadIdx.x; i < len; i += BLOCK) key[run.first + i] = s_key[i];
}

// one step (k, j) of the network over every run of the global tier: grid = (pair blocks of the longest run, runs)
__global__ void __launch_bounds__(BLOCK) k_propt_sort_step(const PropTRun *runs, uint64_t *key, uint32_t k, uint32_t j) {
    const PropTRun run = runs[blockIdx.y];
    uint32_t P = 1;
    while (P < run.len) P <<= 1;
    if (k > P) return; // this run is sorted already: the longest one sets the number of steps
    for (uint32_t p = blockIdx.x * BLOCK + threadIdx.x; p < (P >> 1); p += gridDim.x * BLOCK) {
        const PropTPair pr = propt_pair(p, k, j);
        if (pr.hi < run.len) {
            const uint64_t a = key[run.first + pr.lo], b = key[run.first + pr.hi];
            if (a > b) { key[run.first + pr.lo] = b; key[run.first + pr.hi] = a; }
        }
    }
}

__global__ void __launch_bounds__(BLOCK) k_propt_fill(const uint64_t *key, uint64_t entries, const int64_t *row_ptr, uint32_t nq, const uint64_t *held_fix,
                                                      int32_t *rows, uint64_t *fix) {
    for (uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; p < entries; p += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t kk = key[p];
        const uint32_t i = (uint32_t)(kk >> 32);
        if (i >= nq) continue; // (a key nobody wrote: cannot happen with counts and places of one result)
        const uint64_t at = (uint64_t)row_ptr[i] + (kk & 0xFFFFFFFFull);
        if (at >= entries) continue;
        rows[p] = (int32_t)i;
        fix[p] = held_fix[at];
    }
}

// One lane per transposed entry p.  v = the column that holds p: the last v with col_ptr[v] <= p (empty columns repeat a
// value, the last of them is the one with entries).  A held row lists its ids in ascending order and each once, so the
// place of v in row rows[p] is one lower-bound search.  pos[p] is 0, a place that exists, where the tables disagree (they
// cannot: both come from one held result).
__global__ void __launch_bounds__(BLOCK) k_propt_pos(const int64_t *col_ptr, uint32_t n, const int32_t *rows, const int64_t *row_ptr, uint32_t nq,
                                                     const int32_t *ids, uint64_t entries, int64_t *pos) {
    for (uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; p < entries; p += (uint64_t)gridDim.x * BLOCK) {
        uint32_t lo = 0, hi = n; // col_ptr[lo] <= p < col_ptr[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if ((uint64_t)col_ptr[mid] <= p) lo = mid; else hi = mid;
        }
        const int32_t v = (int32_t)lo;
        const uint32_t i = (uint32_t)rows[p];
        int64_t at = 0;
        if (i < nq) {
            int64_t a = row_ptr[i], b = row_ptr[i + 1];
            const int64_t end = b;
            while (a < b) {
                const int64_t mid = a + (b - a) / 2;
                if (ids[mid] < v) a = mid + 1; else b = mid;
            }
            if (a < end && (uint64_t)a < entries && ids[a] == v) at = a;
        }
        pos[p] = at;
    }
}

} // namespace fora
