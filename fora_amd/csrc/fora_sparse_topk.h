// fora_sparse_topk.h -- device side of the top-k sparse rows (the SPARSE RESULTS, TOP-K contract of include/fora_hip.h;
// DESIGN.md 5.14).  Included by fora_hip.hip behind fora_kernels.h (sp_mbcnt, wave_excl_scan) and fora_topk_plan.h.
//
// The candidates of a chunk of rows lie in a scratch CSR that k_sparse_write left: per row the support in ascending id
// order, (id, word).  One workgroup takes one row (TopkRow).  A row that keeps everything is copied.  A row that is cut
// keeps the `keep` entries that come first in (word descending, id ascending) and holds them in id order:
//   1. radix select over the 64-bit words, most significant byte first, all eight bytes (a word may be 2^62 or, for a seed
//      set, slightly above: no byte is assumed empty).  Each pass counts the byte of the words that agree with the bytes
//      found so far into a 256-bin LDS histogram; wave 0 scans the bins from 255 down, picks the bin that holds the
//      keep-th largest word and takes off the entries above it.  After the last pass the prefix is vk, the keep-th largest
//      word, and `need` is the number of entries equal to vk still to take (at least 1).
//   2. one ordered compaction in position order: every entry with word > vk, and the first `need` with word == vk.  The
//      candidates ascend by id, so "first by position" is "ties by ascending id" and the output ascends by id.
// LDS tier (template LDS): the words are staged once in dynamic LDS and all nine passes read them there; global tier: they
// are re-read from the scratch.  The ids are read once, by the lanes that keep their entry.  Integers only.
// A wave whose live lanes all hold one byte value adds its count with ONE atomic (rows of equal words, and the upper
// bytes of every row of small words, where all lanes would otherwise queue on one bin).
// Entry offsets are 64-bit (a call holds more than 2^32 entries at LiveJournal size); every load is 8 or 4 bytes, so a
// row may start at any entry of the scratch.
#pragma once

namespace fora {

constexpr int TK_WAVES = (int)TOPK_BLOCK / 64;

// grid = rows of the launch; dynamic LDS (LDS tier): 8 bytes per word of the launch's longest staged row.
// ccap / cap: entries the scratch / the held arrays hold (nothing is read or written beyond them)
template <bool LDS>
__global__ void __launch_bounds__(TOPK_BLOCK) k_topk_rows(const TopkRow *rows, const int32_t *cid, const uint64_t *cfix, uint64_t ccap,
                                                          int32_t *ids, uint64_t *fix, uint64_t cap) {
    extern __shared__ __attribute__((aligned(16))) uint64_t tk_words[];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_cnt[2][TK_WAVES][2];
    __shared__ uint32_t s_sel[2];
    const TopkRow r = rows[blockIdx.x];
    const uint32_t len = r.len, keep = r.keep;
    if (keep > len || r.cand + len > ccap || r.out + keep > cap) return; // (the same in every lane)
    const int32_t *ci = cid + r.cand;
    const uint64_t *cw = cfix + r.cand;
    int32_t *oi = ids + r.out;
    uint64_t *ow = fix + r.out;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (keep == len) { // nothing to cut
        for (uint32_t i = tid; i < len; i += TOPK_BLOCK) { oi[i] = ci[i]; ow[i] = cw[i]; }
        return;
    }
    if (LDS) {
        for (uint32_t i = tid; i < len; i += TOPK_BLOCK) tk_words[i] = cw[i];
        __syncthreads();
    }
    const auto word = [&](uint32_t i) -> uint64_t { return LDS ? tk_words[i] : cw[i]; };

    // 1. vk and need
    uint64_t prefix = 0;
    uint32_t need = keep;
    for (int b = 7; b >= 0; b--) {
        const int sh = 8 * b;
        const uint64_t above = b == 7 ? 0ull : ~0ull << (sh + 8); // the bytes found so far
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        for (uint32_t i0 = 0; i0 < len; i0 += TOPK_BLOCK) { // (every lane of a wave makes every trip: ballots inside)
            const uint32_t i = i0 + tid;
            const bool in = i < len;
            const uint64_t x = in ? word(i) : 0;
            const bool live = in && ((x ^ prefix) & above) == 0;
            const uint32_t dg = (uint32_t)(x >> sh) & 255u;
            const unsigned long long m = __ballot(live);
            if (m) {
                const int fl = __ffsll((long long)m) - 1;
                const uint32_t d0 = (uint32_t)__shfl((int)dg, fl);
                const unsigned long long same = __ballot(live && dg == d0);
                if (same == m) { if ((int)lane == fl) atomicAdd(&s_hist[d0], (uint32_t)__popcll(m)); }
                else if (live) atomicAdd(&s_hist[dg], 1u);
            }
        }
        __syncthreads();
        if (w == 0) { // lane l: the bins 255 - 4l down to 252 - 4l
            const uint32_t top = 255u - 4u * lane;
            const uint32_t h0 = s_hist[top], h1 = s_hist[top - 1], h2 = s_hist[top - 2], h3 = s_hist[top - 3];
            const uint32_t s = h0 + h1 + h2 + h3;
            uint32_t tot;
            const uint32_t excl = wave_excl_scan(s, tot);
            if (excl < need && need <= excl + s) { // one lane: need <= the live words
                uint32_t a = excl, d = top;
                if (need > a + h0) { a += h0; d = top - 1;
                    if (need > a + h1) { a += h1; d = top - 2;
                        if (need > a + h2) { a += h2; d = top - 3; } } }
                s_sel[0] = d; s_sel[1] = need - a;
            }
        }
        __syncthreads();
        prefix |= (uint64_t)s_sel[0] << sh;
        need = s_sel[1];
    }
    const uint64_t vk = prefix;

    // 2. the kept entries in position order
    uint32_t out = 0, eqb = 0; // entries written and words equal to vk seen, in the tiles before this one
    for (uint32_t i0 = 0, t = 0; i0 < len && out < keep; i0 += TOPK_BLOCK, t++) {
        const uint32_t i = i0 + tid;
        const bool in = i < len;
        const uint64_t x = in ? word(i) : 0;
        const bool gt = in && x > vk, eq = in && x == vk;
        const unsigned long long mg = __ballot(gt), me = __ballot(eq);
        const int par = (int)(t & 1);
        if (lane == 0) { s_cnt[par][w][0] = (uint32_t)__popcll(mg); s_cnt[par][w][1] = (uint32_t)__popcll(me); }
        __syncthreads();
        uint32_t gb = 0, eb = 0, gt_t = 0, eq_t = 0;
#pragma unroll
        for (int j = 0; j < TK_WAVES; j++) {
            const uint32_t g = s_cnt[par][j][0], e = s_cnt[par][j][1];
            if (j < (int)w) { gb += g; eb += e; }
            gt_t += g; eq_t += e;
        }
        const uint32_t eq_rank = eqb + eb + sp_mbcnt(me);    // words equal to vk in front of mine, in the whole row
        const uint32_t taken_eq = min(eq_rank, need) - min(eqb, need); // ... that this tile keeps
        const uint32_t pos = out + gb + sp_mbcnt(mg) + taken_eq;
        if ((gt || (eq && eq_rank < need)) && pos < keep) { oi[pos] = ci[i]; ow[pos] = x; }
        out += gt_t + (min(eqb + eq_t, need) - min(eqb, need));
        eqb += eq_t;
    }
}

} // namespace fora
