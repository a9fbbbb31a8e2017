// fora_tables.h -- every derived form of a graph that the kernels read, computed on the host from (n, row_ptr, col) and
// explicit arguments.  Pure integer code: no HIP, no context, no options struct -- fora_hip.hip decides which tables a
// graph gets and uploads them, tests/tables_check.cpp builds them without a GPU and restates the kernels' reading of each.
#pragma once
#include "fora_consts.h"

#include <algorithm>
#include <cstddef>
#include <vector>

namespace fora {

// ---- shared steps

inline std::vector<uint32_t> in_degrees(size_t n, const int32_t *col, size_t nnz) {
    std::vector<uint32_t> indeg(n, 0);
    for (size_t e = 0; e < nnz; e++) indeg[(size_t)col[e]]++;
    return indeg;
}
// the H nodes of largest in-degree, ties to the lower id; in that order
inline std::vector<uint32_t> top_by_indegree(const std::vector<uint32_t> &indeg, size_t H) {
    std::vector<uint32_t> order(indeg.size());
    for (size_t v = 0; v < order.size(); v++) order[v] = (uint32_t)v;
    H = std::min(H, order.size());
    std::partial_sort(order.begin(), order.begin() + (ptrdiff_t)H, order.end(),
                      [&](uint32_t a, uint32_t b) { return indeg[a] != indeg[b] ? indeg[a] > indeg[b] : a < b; });
    order.resize(H);
    return order;
}
// `count` values of `bits` bits each (bits <= 32), entry e = value_of(e) at bit e * bits, asked for in order.  Two words of
// padding: a reader takes the two aligned dwords at (word, word + 1), or one unaligned dword, of an entry -- and of the
// position behind the last one
template <class F> std::vector<uint32_t> pack_bits(uint64_t count, uint32_t bits, F value_of) {
    std::vector<uint32_t> pk((size_t)((count * bits + 31) / 32) + 2, 0);
    for (uint64_t e = 0; e < count; e++) {
        const uint64_t at = e * bits;
        const uint64_t x = (uint64_t)(uint32_t)value_of(e) << (at & 31);
        pk[at >> 5] |= (uint32_t)x;
        pk[(at >> 5) + 1] |= (uint32_t)(x >> 32);
    }
    return pk;
}

// ---- row basics (Dev::rowinfo, Dev::deg)

struct RowBasics {
    bool ok = true; // false: an out-degree over 2^32
    std::vector<uint64_t> rowinfo; // (first edge << 24) | min(outdeg, DEG_SAT)
    std::vector<uint32_t> deg;
    int64_t n_dangling = 0;
};
inline RowBasics make_row_basics(int32_t n, const int64_t *row_ptr) {
    RowBasics r;
    r.rowinfo.resize((size_t)n);
    r.deg.resize((size_t)n);
    for (int32_t v = 0; v < n; v++) {
        const uint64_t dg = (uint64_t)(row_ptr[v + 1] - row_ptr[v]);
        r.n_dangling += dg == 0;
        if (dg > 0xFFFFFFFFull) { r.ok = false; return r; }
        r.deg[(size_t)v] = (uint32_t)dg;
        r.rowinfo[(size_t)v] = ((uint64_t)row_ptr[v] << 24) | std::min<uint64_t>(dg, DEG_SAT);
    }
    return r;
}

// ---- compact walk copy (Dev::rp32, Dev::colp; colp_at): 32-bit row offsets and the bit-packed col; for nnz < 2^31

struct CompactWalk {
    uint32_t bits = 0;
    std::vector<uint32_t> rp32, colp;
};
inline CompactWalk make_compact_walk(int32_t n, const int64_t *row_ptr, const int32_t *col) {
    CompactWalk w;
    w.bits = 1;
    while ((1ull << w.bits) < (uint64_t)n) w.bits++;
    if (w.bits > 31) w.bits = 31;
    w.rp32.resize((size_t)n + 1);
    for (int32_t v = 0; v <= n; v++) w.rp32[(size_t)v] = (uint32_t)row_ptr[v];
    w.colp = pack_bits((uint64_t)row_ptr[n], w.bits, [&](uint64_t e) { return col[e]; });
    return w;
}

// ---- degree-grouped walk copy (WalkDG, fora_kernels.h; k_walk_dg, stage_flush<.., XLD>, k_accum<true>): H hub records + at
// most 255 out-degree classes whose tables fit a workgroup's LDS share

constexpr size_t WALK_DG_LDS_CAP = 28 * 1024; // static + dynamic LDS of k_walk_dg stay under 64 KB
// k_walk_dg's tables in dynamic LDS as the launch lays them out: hub sums (bucket-order results only) | 16-byte records | block -> class bytes
inline size_t walk_dg_lds_bytes(uint32_t H, uint32_t nrec, uint32_t nblk, bool xl) {
    return (xl ? (size_t)((H + 1) & ~1u) * 8 : 0) + (size_t)4 * nrec * 4 + (((size_t)nblk + 3) & ~(size_t)3);
}
struct DgTables {
    bool have = false; // false: this graph gets no such copy (no hub count leaves <= 255 classes, tables over the LDS cap, ids over 31 bits)
    uint32_t H = 0, nrec = 0, ts = 0, bits = 0, zero_first = 0, bits32 = 0;
    uint32_t np = 0; // copy ids in use (with padding)
    std::vector<uint32_t> perm, inv, rec, colp;
    std::vector<uint8_t> T; // padded to whole dwords: WalkDG::nblk = T.size()
    uint32_t nbx = 0, nbx_magic = 0; // nbx == 0: no bucket order (it would need more than MAX_BINS bins), invb empty
    std::vector<uint32_t> invb;
};
// dg_hubs > 0: at least that many hub records
inline DgTables make_walk_dg(int32_t n, const int64_t *row_ptr, const int32_t *col, int64_t dg_hubs) {
    DgTables t;
    const uint64_t nnz = (uint64_t)row_ptr[n];
    std::vector<uint32_t> order((size_t)n); // nodes by (out-degree descending, id ascending)
    for (int32_t v = 0; v < n; v++) order[(size_t)v] = (uint32_t)v;
    auto degree = [&](uint32_t v) { return (uint32_t)(row_ptr[v + 1] - row_ptr[v]); };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return degree(a) > degree(b); });
    // smallest hub count that leaves at most 255 distinct degrees behind it
    uint32_t H = 0, K = 0;
    for (uint32_t h : {256u, 512u, 1024u, 2048u, 4096u}) {
        if (dg_hubs > 0 && (int64_t)h < dg_hubs) continue;
        const uint32_t hh = std::min<uint32_t>(h, (uint32_t)n);
        uint32_t k = 0;
        for (size_t i = hh; i < (size_t)n; i++) if (i == hh || degree(order[i]) != degree(order[i - 1])) k++;
        if (k <= 255) { H = hh; K = k; break; }
    }
    if (H == 0 && !(n <= 256)) return DgTables{};
    if (n <= 256) { H = (uint32_t)n; K = 0; }
    uint32_t ts = 6;
    while ((((uint64_t)n + 256ull * (1ull << ts)) >> ts) > 8192) ts++; // at most 8192 blocks (8 KB of LDS)
    const uint32_t blk = 1u << ts;
    const uint32_t nrec = H + K;
    t.rec.assign((size_t)3 * nrec, 0);
    t.perm.resize((size_t)n);
    uint32_t *first = t.rec.data(), *rdeg = t.rec.data() + nrec, *base = t.rec.data() + 2 * (size_t)nrec;
    uint64_t edge = 0;
    uint32_t id = 0, zero_first = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < H; i++) { // hubs: one record each
        const uint32_t v = order[i];
        t.perm[v] = id; first[i] = id; rdeg[i] = degree(v); base[i] = (uint32_t)edge;
        if (rdeg[i] == 0 && zero_first == 0xFFFFFFFFu) zero_first = id;
        edge += rdeg[i]; id++;
    }
    uint32_t k = 0;
    for (size_t i = H; i < (size_t)n;) { // classes, each padded to whole blocks
        size_t j = i;
        const uint32_t dg = degree(order[i]);
        while (j < (size_t)n && degree(order[j]) == dg) j++;
        const uint32_t r = H + k;
        first[r] = id; rdeg[r] = dg; base[r] = (uint32_t)edge;
        if (dg == 0 && zero_first == 0xFFFFFFFFu) zero_first = id;
        for (size_t u = i; u < j; u++) t.perm[order[u]] = id + (uint32_t)(u - i);
        const uint32_t cnt = (uint32_t)(j - i), padded = (cnt + blk - 1) / blk * blk;
        for (uint32_t b = 0; b < padded / blk; b++) t.T.push_back((uint8_t)k);
        edge += (uint64_t)cnt * dg;
        id += padded;
        i = j; k++;
    }
    const uint32_t np = id;
    if (zero_first == 0xFFFFFFFFu) zero_first = np;
    // every id from zero_first on must be dangling: degrees descend, so the zero class (if any) is the last one
    uint32_t bits = 1;
    while ((1ull << bits) < (uint64_t)np) bits++;
    const size_t lds = (size_t)(H + 1) * 8 + (size_t)4 * nrec * 4 + t.T.size() + 4; // hub sums | 16-byte records | block -> class bytes, as the launch lays them out
    if (lds > WALK_DG_LDS_CAP || bits > 31) return DgTables{};
    t.inv.assign((size_t)np, 0);
    for (int32_t v = 0; v < n; v++) t.inv[t.perm[(size_t)v]] = (uint32_t)v;
    { // rows in copy-id order, file order inside a row
        uint32_t x = 0;
        int64_t f = 0, fend = 0; // the row being packed; x: the next copy id
        t.colp = pack_bits(nnz, bits, [&](uint64_t) {
            for (; f == fend; x++) {
                const uint32_t v = t.inv[x];
                if (t.perm[v] == x) { f = row_ptr[v]; fend = row_ptr[v + 1]; } // (else: a padding id)
            }
            return t.perm[(size_t)col[f++]];
        });
    }
    while (t.T.size() & 3) t.T.push_back(0);
    if (t.T.empty()) t.T.assign(4, 0);
    // bucket order of the ids behind the hubs: 64-id blocks dealt round-robin to nbx bins
    const uint32_t nblk64 = (np - H + 63) / 64;
    const uint32_t nbx = std::max<uint32_t>(2, (nblk64 + 127) / 128); // (2 at least: floor(2^32 / nbx) + 1 must fit 32 bits)
    if (nbx <= (uint32_t)MAX_BINS) {
        t.invb.assign((size_t)nbx * BIN_SIZE, 0);
        for (uint32_t x = H; x < np; x++) {
            const uint32_t u = x - H, b64 = u >> 6;
            t.invb[((size_t)(b64 % nbx) << BIN_SHIFT) | ((b64 / nbx) << 6) | (u & 63u)] = t.inv[x];
        }
        t.nbx = nbx;
    }
    t.nbx_magic = (uint32_t)((1ull << 32) / nbx) + 1;
    t.H = H; t.nrec = nrec; t.ts = ts; t.bits = bits; t.zero_first = zero_first; t.np = np;
    t.bits32 = nnz * bits < (1ull << 32) ? 1 : 0;
    t.have = true;
    return t;
}

// ---- hub pre-aggregation (Dev::col_hub; k_pushq_bin<.., HUB>, k_push_tail): the `want` nodes of largest in-degree, numbered
// in id order so that the hubs of a bin are a contiguous range, and a copy of col that names them by that number

struct HubTables {
    std::vector<uint32_t> hub_node;  // [H = min(want, n)] ascending
    std::vector<uint32_t> hub_first; // [bins + 1] first hub of every bin of 2^shift nodes
    std::vector<int32_t> col_hub;    // 0x80000000 | hub number for a hub, the target otherwise
};
inline HubTables make_hub_tables(int32_t n, const int32_t *col, size_t nnz, size_t want, int shift) {
    HubTables t;
    t.hub_node = top_by_indegree(in_degrees((size_t)n, col, nnz), want);
    std::sort(t.hub_node.begin(), t.hub_node.end());
    std::vector<uint32_t> hub_of((size_t)n, 0xFFFFFFFFu);
    for (size_t h = 0; h < t.hub_node.size(); h++) hub_of[t.hub_node[h]] = (uint32_t)h;
    const size_t nbins = (size_t)(((uint64_t)n + (1ull << shift) - 1) >> shift);
    t.hub_first.assign(nbins + 1, 0);
    for (uint32_t v : t.hub_node) t.hub_first[(v >> shift) + 1]++;
    for (size_t b = 0; b < nbins; b++) t.hub_first[b + 1] += t.hub_first[b];
    t.col_hub.resize(nnz);
    for (size_t e = 0; e < nnz; e++) {
        const uint32_t h = hub_of[(size_t)col[e]];
        t.col_hub[e] = h == 0xFFFFFFFFu ? col[e] : (int32_t)(0x80000000u | h);
    }
    return t;
}

// ---- quad row table (Dev::rowinfo4; k_pad_quads, k_pushq_bin<.., QUAD>): rows padded to whole quads of four edges

struct QuadRows {
    std::vector<uint64_t> rowinfo4; // (first quad << 24) | min(outdeg, DEG_SAT)
    uint64_t quads = 0;
};
inline QuadRows make_quad_rows(int32_t n, const int64_t *row_ptr) {
    QuadRows t;
    t.rowinfo4.resize((size_t)n);
    for (int32_t v = 0; v < n; v++) {
        const uint64_t dg = (uint64_t)(row_ptr[v + 1] - row_ptr[v]);
        t.rowinfo4[(size_t)v] = (t.quads << 24) | std::min<uint64_t>(dg, DEG_SAT);
        t.quads += (dg + 3) / 4;
    }
    return t;
}

// ---- row split (Dev::col_push, Dev::row_split; k_pushq_bin<.., SPLIT>): every pass reads only its own part of a popped row

struct SplitTables {
    std::vector<int32_t> col_sorted; // every row of col ascending; empty: the rows are sorted as loaded
    std::vector<uint32_t> split;     // [n][npass + 1] first position of a row whose target is >= (p * pbins) << shift
};
inline SplitTables make_row_split(int32_t n, const int64_t *row_ptr, std::vector<int32_t> col, int npass, int pbins, int shift) {
    SplitTables t;
    bool sorted = true;
    for (int32_t v = 0; v < n && sorted; v++)
        for (int64_t e = row_ptr[v] + 1; e < row_ptr[v + 1]; e++)
            if (col[(size_t)e - 1] > col[(size_t)e]) { sorted = false; break; }
    if (!sorted)
        for (int32_t v = 0; v < n; v++) std::sort(col.begin() + row_ptr[v], col.begin() + row_ptr[v + 1]);
    t.split.resize((size_t)n * (size_t)(npass + 1));
    for (int32_t v = 0; v < n; v++) {
        const int32_t *rb = col.data() + row_ptr[v], *re = col.data() + row_ptr[v + 1];
        uint32_t *sp = t.split.data() + (size_t)v * (size_t)(npass + 1);
        sp[0] = 0;
        for (int p = 1; p < npass; p++) {
            const int64_t first_node = ((int64_t)p * pbins) << shift;
            sp[p] = (uint32_t)(std::lower_bound(rb, re, (int32_t)std::min<int64_t>(first_node, INT32_MAX)) - rb);
        }
        sp[npass] = (uint32_t)(re - rb);
    }
    if (!sorted) t.col_sorted = std::move(col);
    return t;
}

// ---- team push (TeamDev, fora_team.h; k_push_team): members per team, the copy of col that names every target as (owner,
// local id) and the exact bucket capacities; for 0 < nnz < 2^32 and n <= 2^19

struct TeamLayout {
    uint32_t T = 0, R = 0, H = 0; // members per team (0: no team push for this graph), local ids per member, hubs
    uint64_t cap = 0;             // message slots per (team, parity) = off[T * T]
    std::vector<uint32_t> n2l, l2n, rowq, hubtgt, colt, off; // rowq: [n + 1]; hubtgt: one entry at least
    std::vector<uint16_t> deg16;
    std::vector<uint64_t> rowl;
};
// force: members at least (0: the fewest); max_members: at most (TEAM_MAX, the device's CUs); hubs_opt: hubs wanted
inline TeamLayout make_team_layout(int32_t n_, const int64_t *row_ptr, const int32_t *col, uint32_t force, uint32_t max_members, uint32_t hubs_opt) {
    TeamLayout t;
    const size_t n = (size_t)n_, nnz = (size_t)row_ptr[n_];
    const std::vector<uint32_t> indeg = in_degrees(n, col, nnz);
    // members per team: the fewest (a power of two) whose LDS holds their share of the nodes that have in-edges
    uint32_t T = 1;
    while (T < force) T *= 2;
    std::vector<uint32_t> cntm;
    uint32_t R = 0;
    for (;; T *= 2) {
        if (T > max_members) return TeamLayout{}; // too large for the team path
        cntm.assign(T, 0);
        for (size_t v = 0; v < n; v++) if (indeg[v]) cntm[(v >> 6) % T]++;
        R = (*std::max_element(cntm.begin(), cntm.end()) + 63) / 64 * 64;
        if (R == 0) R = 64;
        if (R <= TEAM_R_CAP) break;
    }
    t.n2l.assign(n, TEAM_EMPTY); t.l2n.assign((size_t)T * R, TEAM_EMPTY);
    t.deg16.assign((size_t)T * R, 0);
    t.rowl.assign((size_t)T * R, 0);
    std::fill(cntm.begin(), cntm.end(), 0);
    for (size_t v = 0; v < n; v++) {
        if (!indeg[v]) continue;
        const uint32_t s = (uint32_t)((v >> 6) % T), l = cntm[s]++;
        t.n2l[v] = (s << TEAM_LBITS) | l;
        t.l2n[(size_t)s * R + l] = (uint32_t)v;
        const int64_t dg = row_ptr[v + 1] - row_ptr[v];
        t.deg16[(size_t)s * R + l] = (uint16_t)std::min<int64_t>(dg, 0xFFFF);
        t.rowl[(size_t)s * R + l] = (uint64_t)v | ((uint64_t)std::min<int64_t>(dg, 8191) << 19); // n <= 2^19; the row's first quad (<< 32) follows below
    }
    // rows of the team copy are padded to whole quads (four words, 16-byte aligned): a lane reads a quad with one load
    t.rowq.assign(n + 1, 0);
    for (size_t v = 0; v < n; v++) t.rowq[v + 1] = t.rowq[v] + (uint32_t)((row_ptr[v + 1] - row_ptr[v] + 3) / 4); // (< 2^32: nnz < 2^32)
    for (size_t v = 0; v < n; v++)
        if (t.n2l[v] != TEAM_EMPTY) t.rowl[(size_t)(t.n2l[v] >> TEAM_LBITS) * R + (t.n2l[v] & TEAM_LMASK)] |= (uint64_t)t.rowq[v] << 32;
    // hubs: the nodes of largest in-degree (ties: lower id); their sums travel as one message per member and level
    // (their LDS sums share the 160 KiB with the residues and ~23 KB of static arrays)
    const uint64_t lds_left = 163840 / TEAM_WGS_PER_CU - 23 * 1024 - ((uint64_t)R + 1) * 8;
    const uint32_t Hn = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(hubs_opt, n), lds_left / 8);
    std::vector<uint32_t> hub_of(n, TEAM_EMPTY);
    std::vector<uint8_t> hub_ok(std::max<uint32_t>(1, Hn), 0);
    t.hubtgt.assign(std::max<uint32_t>(1, Hn), 0);
    if (Hn) {
        const std::vector<uint32_t> top = top_by_indegree(indeg, Hn);
        for (uint32_t h = 0; h < Hn; h++) if (indeg[top[h]]) { hub_of[top[h]] = h; t.hubtgt[h] = t.n2l[top[h]]; hub_ok[h] = 1; }
    }
    t.colt.assign((size_t)t.rowq[n] * 4, TEAM_EMPTY);
    std::vector<uint64_t> pair((size_t)T * T, 0);
    for (size_t v = 0; v < n; v++) {
        const uint32_t s = (uint32_t)((v >> 6) % T);
        for (int64_t e = row_ptr[v]; e < row_ptr[v + 1]; e++) {
            const uint32_t tg = (uint32_t)col[(size_t)e], w = t.n2l[tg];
            t.colt[(size_t)t.rowq[v] * 4 + (size_t)(e - row_ptr[v])] = hub_of[tg] != TEAM_EMPTY ? (0x80000000u | hub_of[tg]) : w;
            if (hub_of[tg] == TEAM_EMPTY) pair[(size_t)s * T + (w >> TEAM_LBITS)]++;
        }
    }
    for (uint32_t h = 0; h < Hn; h++) // a member sends a hub at most one message per level
        if (hub_ok[h]) for (uint32_t s = 0; s < T; s++) pair[(size_t)s * T + (t.hubtgt[h] >> TEAM_LBITS)]++;
    // bucket (s -> d): one 4-byte message per edge + the dangling mass of the level; whole 64-byte lines
    t.off.assign((size_t)T * T + 1, 0);
    uint64_t at = 0;
    for (size_t i = 0; i < (size_t)T * T; i++) {
        t.off[i] = (uint32_t)at;
        at += (pair[i] + 1 + 15) & ~15ull;
        if (at >= (1ull << 32) || pair[i] + 1 >= (1ull << 24)) return TeamLayout{}; // 32-bit slots; a bucket's count is 24 bits of its barrier word: no team push for such a graph
    }
    t.off[(size_t)T * T] = (uint32_t)at;
    t.T = T; t.R = R; t.H = Hn; t.cap = at;
    return t;
}

} // namespace fora
