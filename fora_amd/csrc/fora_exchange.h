// fora_exchange.h -- the chunk-binned exchange into per-workgroup sub-buckets (Dev::bk_w, bk_inc, bk_count), stated once.
//
// Every (slot, bin) bucket is cut into `sub` sub-buckets, one per producer workgroup of the slot (see Dev::bk_w): producer
// workgroup x of slot q owns sub-bucket x of every bin, keeps its fill counters in LDS and appends without a global atomic.
// Sub-bucket (slot q, bin b of the pass, workgroup x) has the number
//     s = (q * pbins + b) * sub + x :   count word bk_count[s],  messages bk_w / bk_inc[s * bk_cap + i], i < bk_cap
// (plan_workspace sizes the arrays: slots * pbins * sub sub-buckets of bk_cap messages).  Producers: k_pushq_bin and
// k_walk_idx (BinExchange below), the staged walk kernels (stage_flush: wave-level runs, the same sub-buckets).  Consumer:
// k_accum, which reads the `sub` counts of its bucket and zeroes them.
//
// Included by fora_kernels.h behind Dev and the block scans; not a header of its own.
#pragma once

namespace fora {

// Producer's view: the sub-buckets of workgroup x of slot q, one per bin of the pass.
struct SubBuckets {
    uint32_t *cnt;   // count word of bin b: cnt[b * sub]
    uint64_t first;  // message i of bin b: first + b * stride + i
    uint64_t stride;
    uint32_t sub;
    // (Dev's fields come by value: the QUAD bin kernels hand their by-value Dev to no function, and doing so here cost them 14 to 19 SGPR spills)
    static __device__ __forceinline__ uint64_t first_of(int32_t pbins, uint32_t sub, uint32_t bk_cap, int q, uint32_t x) { return ((uint64_t)q * pbins * sub + x) * bk_cap; }
    static __device__ __forceinline__ uint64_t stride_of(uint32_t sub, uint32_t bk_cap) { return (uint64_t)sub * bk_cap; }
    __device__ __forceinline__ SubBuckets(uint32_t *bk_count, int32_t pbins, uint32_t sub_, uint32_t bk_cap, int q, uint32_t x)
        : cnt(bk_count + (uint64_t)q * pbins * sub_ + x), first(first_of(pbins, sub_, bk_cap, q, x)), stride(stride_of(sub_, bk_cap)), sub(sub_) {}
    __device__ __forceinline__ uint32_t &count(uint32_t b) const { return cnt[(uint64_t)b * sub]; }
    __device__ __forceinline__ uint64_t at(uint32_t b, uint32_t pos) const { return first + (uint64_t)b * stride + pos; }
};

// Consumer's view: bucket (q, b) is the sub-buckets number s0 .. s0 + sub - 1.  (D: Dev by value or through the kernarg segment.)
struct Bucket {
    uint64_t s0;
    template <class D, class B>
    __device__ __forceinline__ Bucket(const D &d, int q, B b) : s0(((uint64_t)q * d.pbins + b) * d.sub) {}
    __device__ __forceinline__ uint64_t count(uint32_t x) const { return s0 + x; } // index into bk_count
    __device__ __forceinline__ uint64_t first(uint32_t bk_cap) const { return s0 * bk_cap; } // index into bk_w / bk_inc of sub-bucket 0; sub-bucket x: + x * bk_cap
};

// The producer steps of one workgroup of NT threads over up to NB bins, on the caller's __shared__ arrays:
//   s_cnt[NB]      messages of the chunk per bin (an LDS histogram: rank() hands out the ranks inside a (chunk, bin) run)
//   s_lofs[NB + 1] first stage slot of every bin: the chunk's messages lie bin by bin in the caller's stage
//   s_fill[NB]     messages the workgroup has put into its sub-bucket of the bin so far
//   s_w[NT / 64]   scratch of the block scan
// A chunk goes: rank() every message -- barrier -- layout() -- barrier -- the caller writes message (b, rank) to stage slot
// slot(b, rank) -- barrier -- staged message m of bin b goes to sub-bucket position pos(b, m), consecutive lanes to
// consecutive positions -- pad_runs().  load_fills() before the first chunk, store_fills() after the last.
//
// THE RULE: layout() advances s_fill[b] by the chunk's run, padded to a multiple of PAD messages (so that a run starts and
// ends on a sector boundary, see FORA_RUN_PAD_WIDE), BEFORE any message of the run is stored.  While a chunk is written
// out s_fill[b] therefore already counts this chunk's padded run: the run starts at s_fill[b] - padded(run).  A position at or
// beyond bk_cap does not exist: the caller sends that message another way (overflow list, direct atomic); the count word may
// exceed bk_cap, k_accum clamps it.
template <int NB, int NT, uint32_t PAD>
struct BinExchange {
    uint32_t (&s_cnt)[NB], (&s_lofs)[NB + 1], (&s_fill)[NB], (&s_w)[NT / 64];
    SubBuckets bk;
    uint32_t bin_cnt; // bins of the pass

    static __device__ __forceinline__ uint32_t padded(uint32_t run) { return (run + (PAD - 1)) & ~(uint32_t)(PAD - 1); }

    // before the first chunk (s_fill before s_cnt: the other order costs the 2560-bin kernels a VGPR) ...
    __device__ __forceinline__ void load_fills() const {
        for (uint32_t i = threadIdx.x; i < (uint32_t)NB; i += NT) {
            s_fill[i] = i < bin_cnt ? bk.count(i) : 0;
            s_cnt[i] = 0;
        }
    }
    // ... and after the last one
    __device__ __forceinline__ void store_fills() const {
        for (uint32_t i = threadIdx.x; i < bin_cnt; i += NT) bk.count(i) = s_fill[i];
    }
    __device__ __forceinline__ bool in_pass(uint32_t b) const { return b < bin_cnt; } // b: bin of the graph - bin_lo; false: another pass's bin, no message
    // one more message for bin b of the pass: its rank inside the (chunk, bin) run
    __device__ __forceinline__ uint32_t rank(uint32_t b) const { return atomicAdd(&s_cnt[b], 1u); }
    // takes sub-bucket space (a counter in LDS, no atomic), lays the bins out in the stage and clears the histogram for
    // the next chunk: lane t owns bins t*PER .. t*PER+PER-1.  Returns the messages of the chunk.
    __device__ __forceinline__ uint32_t layout() const {
        constexpr int PER = (NB + NT - 1) / NT;
        uint32_t c[PER], mine = 0;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const uint32_t b = threadIdx.x * PER + j;
            c[j] = b < bin_cnt && b < (uint32_t)NB ? s_cnt[b] : 0;
            mine += c[j];
        }
        uint32_t ctot;
        uint32_t pre2 = block_excl_scan_n<NT>(mine, s_w, ctot);
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const uint32_t b = threadIdx.x * PER + j;
            if (b < (uint32_t)NB) {
                s_lofs[b] = pre2;
                pre2 += c[j];
                if (c[j]) {
                    s_fill[b] += padded(c[j]);
                    s_cnt[b] = 0;
                }
            }
        }
        if (threadIdx.x == 0) s_lofs[NB] = ctot; // (every thread holds the total)
        return ctot;
    }
    __device__ __forceinline__ uint32_t slot(uint32_t b, uint32_t r) const { return s_lofs[b] + r; }
    __device__ __forceinline__ uint32_t run(uint32_t b) const { return s_lofs[b + 1] - s_lofs[b]; } // messages of this (chunk, bin) run
    // sub-bucket position of staged message m of bin b (see THE RULE)
    __device__ __forceinline__ uint32_t pos(uint32_t b, uint32_t m) const { return s_fill[b] - padded(run(b)) + (m - s_lofs[b]); }
    // null words from the end of every run up to the sector boundary (merged with the run's last sector in L2)
    __device__ __forceinline__ void pad_runs(uint64_t *bk_inc, uint32_t bk_cap) const {
        if (PAD > 1) {
            for (uint32_t b = threadIdx.x; b < bin_cnt; b += NT) {
                const uint32_t crun = run(b), prun = padded(crun);
                for (uint32_t i = crun; i < prun; i++) {
                    const uint32_t p = s_fill[b] - prun + i;
                    if (p < bk_cap) bk_inc[bk.at(b, p)] = 0ull;
                }
            }
        }
    }
};

} // namespace fora
