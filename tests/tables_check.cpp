// tables_check.cpp -- builds every table of fora_amd/csrc/fora_tables.h for one graph on the CPU and checks it against the
// kernels' side of the agreement: each reader below restates, in plain C++, how a kernel function reads the table (named in
// its comment).  Stand-alone (tests/test_tables_cpu.py compiles it with the address and undefined-behaviour sanitizers):
//
//   tables_check <csr file> <shift> <pbins> <team force> <team max members> <team hubs> <push hubs> <dg_hubs> [tables]
//
// `tables` names the ones to check (rows compact dg hubs quads split team; all without it).
// The file holds int64 n, int64 nnz, int64 row_ptr[n + 1], int32 col[nnz], little-endian.  Exit status 0 and one line of
// facts about the branches taken ("key=value ..."), or 1 and one line that names the first property that does not hold.
#include "fora_tables.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace fora;

[[noreturn]] static void failed(const char *what, const char *cond, int line) {
    std::printf("\nFAILED: %s [%s, line %d]\n", what, cond, line);
    std::exit(1);
}
#define CHECK(cond, what) do { if (!(cond)) failed(what, #cond, __LINE__); } while (0)

static uint32_t umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); } // __umulhi

struct Csr {
    int32_t n = 0;
    std::vector<int64_t> row_ptr;
    std::vector<int32_t> col;
    uint32_t deg(size_t v) const { return (uint32_t)(row_ptr[v + 1] - row_ptr[v]); }
    size_t nnz() const { return col.size(); }
};

static Csr read_csr(const char *path) {
    Csr g;
    FILE *f = std::fopen(path, "rb");
    CHECK(f, "graph file opens");
    int64_t head[2];
    CHECK(std::fread(head, 8, 2, f) == 2 && head[0] > 0 && head[0] < (1 << 24) && head[1] >= 0 && head[1] < (1ll << 28), "graph file header");
    g.n = (int32_t)head[0];
    g.row_ptr.resize((size_t)g.n + 1);
    g.col.resize((size_t)head[1]);
    CHECK(std::fread(g.row_ptr.data(), 8, g.row_ptr.size(), f) == g.row_ptr.size(), "graph file row_ptr");
    CHECK(std::fread(g.col.data(), 4, g.col.size(), f) == g.col.size(), "graph file col");
    std::fclose(f);
    CHECK(g.row_ptr[0] == 0 && g.row_ptr[(size_t)g.n] == head[1], "row_ptr spans col");
    for (size_t v = 0; v < (size_t)g.n; v++) CHECK(g.row_ptr[v] <= g.row_ptr[v + 1], "row_ptr monotone");
    for (int32_t t : g.col) CHECK(t >= 0 && t < g.n, "edge target in range");
    return g;
}

// ---- a bit-packed list as the kernels read it

struct Packed {
    const std::vector<uint32_t> &pk;
    uint32_t bits;
    // colp_at, and dg_colp_at<false>: the two aligned dwords at (word, word + 1)
    uint32_t read_pair(uint64_t e) const {
        const uint64_t at = (uint64_t)bits * e, word = at >> 5;
        CHECK(word + 1 < pk.size(), "packed list: the dword pair of an entry lies inside the list");
        const uint64_t both = ((uint64_t)pk[word + 1] << 32) | pk[word];
        return (uint32_t)(both >> (at & 31)) & ((1u << bits) - 1u);
    }
    // dg_colp_at<true>: one unaligned dword at byte at >> 3
    uint32_t read_unaligned(uint64_t e) const {
        const uint64_t at = (uint64_t)bits * e;
        CHECK(at < (1ull << 32), "packed list: bit offsets of the one-dword form fit 32 bits");
        CHECK((at & 7) + bits <= 32, "packed list: one unaligned dword holds an entry");
        CHECK((at >> 3) + 4 <= pk.size() * 4, "packed list: the unaligned dword of an entry lies inside the list");
        uint32_t w;
        std::memcpy(&w, (const char *)pk.data() + (at >> 3), 4);
        return (w >> (at & 7)) & ((1u << bits) - 1u);
    }
};
template <class F> static void check_packed(const std::vector<uint32_t> &pk, uint64_t count, uint32_t bits, bool one_dword, F value_of) {
    CHECK(bits >= 1 && bits <= 31, "packed list: entry width");
    CHECK(pk.size() == (count * bits + 31) / 32 + 2, "packed list: (count * bits + 31) / 32 + 2 words");
    const Packed p{pk, bits};
    for (uint64_t e = 0; e < count; e++) {
        const uint32_t want = value_of(e);
        CHECK(p.read_pair(e) == want, "packed list: an entry read as two aligned dwords is the value packed");
        if (one_dword) CHECK(p.read_unaligned(e) == want, "packed list: an entry read as one unaligned dword is the value packed");
    }
    (void)p.read_pair(count); // (the position behind the last entry: what a move from an out-degree-0 id reads)
    if (one_dword) (void)p.read_unaligned(count);
}

// ---- the checks, table by table

static void check_rows(const Csr &g) {
    const RowBasics r = make_row_basics(g.n, g.row_ptr.data());
    CHECK(r.ok, "row basics: no out-degree over 2^32");
    int64_t dangling = 0;
    for (size_t v = 0; v < (size_t)g.n; v++) {
        CHECK(r.deg[v] == g.deg(v), "row basics: deg");
        CHECK((r.rowinfo[v] >> 24) == (uint64_t)g.row_ptr[v] && (r.rowinfo[v] & DEG_SAT) == std::min<uint32_t>(g.deg(v), DEG_SAT), "row basics: rowinfo = first edge << 24 | min(deg, DEG_SAT)"); // node_row, ri_deg
        dangling += g.deg(v) == 0;
    }
    CHECK(r.n_dangling == dangling, "row basics: dangling count");
    std::printf("dangling=%lld ", (long long)dangling);
}

static void check_compact(const Csr &g) {
    const CompactWalk w = make_compact_walk(g.n, g.row_ptr.data(), g.col.data());
    CHECK((1ull << w.bits) >= (uint64_t)g.n, "compact copy: bits hold every node id");
    CHECK(w.rp32.size() == (size_t)g.n + 1, "compact copy: rp32 has n + 1 entries");
    for (size_t v = 0; v <= (size_t)g.n; v++) CHECK(w.rp32[v] == (uint64_t)g.row_ptr[v], "compact copy: rp32 is row_ptr"); // walk_move
    check_packed(w.colp, g.nnz(), w.bits, false, [&](uint64_t e) { return (uint32_t)g.col[e]; });                          // colp_at
}

static void check_walk_dg(const Csr &g, int64_t dg_hubs) {
    const DgTables t = make_walk_dg(g.n, g.row_ptr.data(), g.col.data(), dg_hubs);
    std::printf("dg_have=%d ", (int)t.have);
    if (!t.have) { CHECK(t.colp.empty() && t.perm.empty(), "walk copy: nothing built when there is no copy"); return; }
    const size_t n = (size_t)g.n;
    const uint32_t H = t.H, ncls = t.nrec - H, nblk = (uint32_t)t.T.size();
    CHECK(H <= t.nrec && ncls <= 255 && t.rec.size() == (size_t)3 * t.nrec, "walk copy: H hub records and at most 255 classes");
    CHECK(nblk >= 4 && nblk % 4 == 0, "walk copy: T is whole dwords, one at least"); // k_walk_dg copies (nblk + 3) / 4 dwords
    // the LDS bytes of the launch (launch_walks: hub sums with XL | 16-byte records | block bytes) stay under the builder's cap
    CHECK((size_t)((H + 1) & ~1u) * 8 + (size_t)16 * t.nrec + (((size_t)nblk + 3) & ~(size_t)3) <= WALK_DG_LDS_CAP, "walk copy: LDS of the launch within the cap");
    // k_walk_dg's LDS order of the records: the classes first, the hubs behind them
    struct Rec { uint32_t first, deg, base; };
    std::vector<Rec> s_rec(t.nrec);
    for (uint32_t i = 0; i < t.nrec; i++) s_rec[i < H ? ncls + i : i - H] = {t.rec[i], t.rec[t.nrec + i], t.rec[2 * (size_t)t.nrec + i]};
    const auto record_of = [&](uint32_t cur) { // k_walk_dg `move`: the record of copy id cur
        uint32_t r = ncls + cur;
        if (cur >= H) {
            CHECK(((cur - H) >> t.ts) < nblk, "walk copy: the block of an id in use is in T");
            r = t.T[(cur - H) >> t.ts];
        }
        CHECK(r < t.nrec, "walk copy: T names a record");
        return s_rec[r];
    };
    CHECK(t.perm.size() == n && t.inv.size() == t.np, "walk copy: perm [n], inv [np]");
    std::vector<uint8_t> used(t.np, 0);
    for (size_t v = 0; v < n; v++) {
        CHECK(t.perm[v] < t.np && !used[t.perm[v]], "walk copy: perm is injective into [0, np)");
        used[t.perm[v]] = 1;
        CHECK(t.inv[t.perm[v]] == v, "walk copy: inv[perm[v]] == v");
    }
    uint32_t prev = 0xFFFFFFFFu;
    for (uint32_t x = 0; x < t.np; x++) {
        if (!used[x]) continue;
        const uint32_t v = t.inv[x];
        if (prev != 0xFFFFFFFFu) CHECK(g.deg(prev) > g.deg(v) || (g.deg(prev) == g.deg(v) && prev < v), "walk copy: ids descend by out-degree, ties in original order");
        prev = v;
    }
    bool any_zero = false;
    for (size_t v = 0; v < n; v++) {
        any_zero |= g.deg(v) == 0;
        CHECK((t.perm[v] >= t.zero_first) == (g.deg(v) == 0), "walk copy: exactly the ids from zero_first on have out-degree 0");
    }
    if (!any_zero) CHECK(t.zero_first == t.np, "walk copy: zero_first == np without a zero class");
    CHECK(t.bits32 == ((uint64_t)g.nnz() * t.bits < (1ull << 32) ? 1u : 0u), "walk copy: bits32");
    const Packed p{t.colp, t.bits};
    for (size_t v = 0; v < n; v++) {
        const Rec rc = record_of(t.perm[v]);
        const uint32_t d = g.deg(v);
        CHECK(rc.deg == d && rc.first <= t.perm[v], "walk copy: the record of an id has its out-degree and starts at or before it");
        const uint32_t e0 = rc.base + (t.perm[v] - rc.first) * d; // `move`: the row's first edge
        for (uint32_t k = 0; k < d; k++) {
            const uint32_t want = t.perm[(size_t)g.col[(size_t)g.row_ptr[v] + k]];
            CHECK(p.read_pair((uint64_t)e0 + k) == want, "walk copy: entry base + (id - first) * deg + k is perm[col[row_ptr[v] + k]]");
            if (t.bits32) CHECK(p.read_unaligned((uint64_t)e0 + k) == want, "walk copy: ... read as one unaligned dword too");
        }
        if (!d) { (void)p.read_pair(e0); if (t.bits32) (void)p.read_unaligned(e0); } // `move` reads before it looks at the degree
    }
    { // the whole list, in copy-id order (covers the list's size and its last words)
        std::vector<uint32_t> want;
        for (uint32_t x = 0; x < t.np; x++)
            if (used[x]) for (int64_t f = g.row_ptr[t.inv[x]]; f < g.row_ptr[t.inv[x] + 1]; f++) want.push_back(t.perm[(size_t)g.col[(size_t)f]]);
        check_packed(t.colp, g.nnz(), t.bits, t.bits32 != 0, [&](uint64_t e) { return want[(size_t)e]; });
    }
    // bucket order: stage_flush<.., XLD> turns (copy id - H) into bin << BIN_SHIFT | local, k_accum<true> reads invb there
    const uint32_t nblk64 = (t.np - H + 63) / 64;
    if (t.nbx) {
        CHECK(t.nbx >= 2 && t.nbx <= (uint32_t)MAX_BINS && t.invb.size() == (size_t)t.nbx * BIN_SIZE, "walk copy: invb holds nbx <= MAX_BINS bins");
        for (uint32_t blk = 0; blk < nblk64; blk++) CHECK(umulhi(blk, t.nbx_magic) == blk / t.nbx, "walk copy: __umulhi(blk, nbx_magic) == blk / nbx");
        std::vector<uint8_t> hit(t.invb.size(), 0);
        for (uint32_t x = H; x < t.np; x++) {
            if (!used[x]) continue;
            const uint32_t u = x - H, blk = u >> 6, qd = umulhi(blk, t.nbx_magic);
            const uint32_t dest = ((blk - qd * t.nbx) << BIN_SHIFT) | (qd << 6) | (u & 63u);
            CHECK(u < (1u << 20) && dest < (1u << 20), "walk copy: an id behind the hubs and its place fit the 20 node bits of a result word");
            CHECK(dest < t.invb.size() && !hit[dest], "walk copy: distinct ids take distinct places inside nbx * BIN_SIZE");
            hit[dest] = 1;
            CHECK(t.invb[dest] == t.inv[x], "walk copy: invb at an id's place is its original id");
        }
    } else CHECK(t.invb.empty(), "walk copy: no invb without a bucket order");
    if (n <= 256) CHECK(H == n && ncls == 0 && nblk == 4 && !(t.T[0] | t.T[1] | t.T[2] | t.T[3]), "walk copy: n <= 256 is all hubs, T four zero bytes");
    std::printf("dg_H=%u dg_ncls=%u dg_np=%u dg_zero_first=%u dg_bits32=%u ", H, ncls, t.np, t.zero_first, t.bits32);
}

// the `count` nodes of largest in-degree, ties to the lower id, by a full sort
static std::vector<uint32_t> top_reference(const std::vector<uint32_t> &indeg, size_t count) {
    std::vector<uint32_t> order(indeg.size());
    for (size_t v = 0; v < order.size(); v++) order[v] = (uint32_t)v;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return indeg[a] > indeg[b]; });
    order.resize(std::min(count, order.size()));
    return order;
}

static void check_hubs(const Csr &g, size_t want, int shift) {
    if (!want || !g.nnz()) return; // (no hub copy is asked for)
    const HubTables t = make_hub_tables(g.n, g.col.data(), g.nnz(), want, shift);
    const size_t n = (size_t)g.n, H = t.hub_node.size();
    CHECK(H == std::min(want, n), "hubs: the count is clipped to n");
    for (size_t h = 1; h < H; h++) CHECK(t.hub_node[h - 1] < t.hub_node[h], "hubs: hub_node ascends");
    std::vector<uint32_t> ref = top_reference(in_degrees(n, g.col.data(), g.nnz()), H);
    std::sort(ref.begin(), ref.end());
    CHECK(ref == t.hub_node, "hubs: the H largest by (in-degree descending, id ascending)");
    const size_t nbins = (n + ((size_t)1 << shift) - 1) >> shift;
    CHECK(t.hub_first.size() == nbins + 1, "hubs: hub_first has bins + 1 entries");
    for (size_t b = 0; b <= nbins; b++) {
        size_t below = 0;
        for (uint32_t v : t.hub_node) below += (v >> shift) < b;
        CHECK(t.hub_first[b] == below, "hubs: hub_first is the prefix count by node >> shift");
    }
    std::vector<uint32_t> hub_of(n, 0xFFFFFFFFu);
    for (size_t h = 0; h < H; h++) hub_of[t.hub_node[h]] = (uint32_t)h;
    CHECK(t.col_hub.size() == g.nnz(), "hubs: col_hub has nnz entries");
    for (size_t e = 0; e < g.nnz(); e++) {
        const uint32_t h = hub_of[(size_t)g.col[e]];
        CHECK((uint32_t)t.col_hub[e] == (h == 0xFFFFFFFFu ? (uint32_t)g.col[e] : 0x80000000u | h), "hubs: col_hub names hubs as 0x80000000 | h, other targets as they are");
    }
    std::printf("hubs_H=%zu ", H);
}

static void check_quads(const Csr &g) {
    const QuadRows t = make_quad_rows(g.n, g.row_ptr.data());
    uint64_t q = 0;
    for (size_t v = 0; v < (size_t)g.n; v++) { // k_pad_quads, k_pushq_bin<.., QUAD>
        CHECK((t.rowinfo4[v] >> 24) == q, "quads: rowinfo4 >> 24 is the running sum of (deg + 3) / 4");
        CHECK((t.rowinfo4[v] & 0xFFFFFFu) == std::min<uint32_t>(g.deg(v), DEG_SAT), "quads: the low 24 bits are min(deg, DEG_SAT)");
        q += ((uint64_t)g.deg(v) + 3) / 4;
    }
    CHECK(t.quads == q, "quads: the total is returned");
    std::printf("quads=%llu ", (unsigned long long)q);
}

static void check_split(const Csr &g, int shift, int pbins) {
    const size_t n = (size_t)g.n;
    const int nbins = (int)((n + ((size_t)1 << shift) - 1) >> shift);
    const int npass = pbins > 0 ? (nbins + pbins - 1) / pbins : 1;
    std::printf("npass=%d ", npass);
    if (npass <= 1) return; // (no split is asked for)
    const SplitTables t = make_row_split(g.n, g.row_ptr.data(), g.col, npass, pbins, shift);
    bool sorted = true;
    for (size_t v = 0; v < n; v++) sorted &= std::is_sorted(g.col.begin() + g.row_ptr[v], g.col.begin() + g.row_ptr[v + 1]);
    CHECK(t.col_sorted.empty() == (sorted || !g.nnz()), "split: no sorted copy exactly when the rows are sorted as loaded");
    const std::vector<int32_t> &col = sorted ? g.col : t.col_sorted;
    CHECK(col.size() == g.nnz() && t.split.size() == n * (size_t)(npass + 1), "split: sizes");
    for (size_t v = 0; v < n; v++) {
        std::vector<int32_t> a(g.col.begin() + g.row_ptr[v], g.col.begin() + g.row_ptr[v + 1]), b(col.begin() + g.row_ptr[v], col.begin() + g.row_ptr[v + 1]);
        CHECK(std::is_sorted(b.begin(), b.end()), "split: every row of the copy ascends");
        std::sort(a.begin(), a.end());
        CHECK(a == b, "split: the copy is a per-row permutation of col");
        const uint32_t *sp = t.split.data() + v * (size_t)(npass + 1);
        CHECK(sp[0] == 0 && sp[npass] == g.deg(v), "split: split[v][0] == 0 and split[v][npass] == deg");
        for (int p = 1; p < npass; p++) { // k_pushq_bin<.., SPLIT>: pass p reads [split[p], split[p + 1])
            uint32_t first = 0;
            while (first < b.size() && (int64_t)b[first] < (((int64_t)p * pbins) << shift)) first++;
            CHECK(sp[p] == first, "split: split[v][p] is the first position whose target is >= (p * pbins) << shift");
        }
    }
    std::printf("split_sorted=%d ", (int)sorted);
}

static void check_team(const Csr &g, uint32_t force, uint32_t max_members, uint32_t hubs_opt) {
    if (!g.nnz()) return;
    const TeamLayout t = make_team_layout(g.n, g.row_ptr.data(), g.col.data(), force, max_members, hubs_opt);
    const size_t n = (size_t)g.n;
    const std::vector<uint32_t> indeg = in_degrees(n, g.col.data(), g.nnz());
    uint32_t T = 1, R = 0;
    while (T < force) T *= 2;
    for (;; T *= 2) {
        if (T > max_members) { T = 0; break; }
        std::vector<uint32_t> share(T, 0);
        for (size_t v = 0; v < n; v++) if (indeg[v]) share[(v >> 6) % T]++;
        R = std::max(64u, (*std::max_element(share.begin(), share.end()) + 63) / 64 * 64);
        if (R <= TEAM_R_CAP) break;
    }
    std::printf("team_T=%u team_R_cap=%u ", t.T, TEAM_R_CAP);
    if (!T) { CHECK(t.T == 0 && t.colt.empty() && t.off.empty(), "team: no tables when no member count within max_members fits"); return; }
    CHECK(t.T == T && t.R == R, "team: T is the smallest power of two >= force whose largest share, rounded to 64, is <= TEAM_R_CAP");
    CHECK(T <= (uint32_t)TEAM_MAX && R <= (1u << TEAM_LBITS) && n <= (1u << 19), "team: owner, local id and node fit their fields");
    CHECK(t.n2l.size() == n && t.l2n.size() == (size_t)T * R && t.rowl.size() == (size_t)T * R && t.deg16.size() == (size_t)T * R && t.rowq.size() == n + 1, "team: sizes");
    size_t with_in = 0, named = 0;
    for (uint32_t w : t.l2n) named += w != TEAM_EMPTY;
    for (size_t v = 0; v < n; v++) {
        CHECK(t.rowq[v + 1] - t.rowq[v] == (g.deg(v) + 3) / 4 && t.rowq[0] == 0, "team: rowq is the running sum of (deg + 3) / 4");
        CHECK((t.n2l[v] == TEAM_EMPTY) == (indeg[v] == 0), "team: n2l is TEAM_EMPTY exactly for in-degree 0");
        if (t.n2l[v] == TEAM_EMPTY) continue;
        with_in++;
        const uint32_t owner = t.n2l[v] >> TEAM_LBITS, local = t.n2l[v] & TEAM_LMASK;
        CHECK(owner == (v >> 6) % T && local < R, "team: owner == (v >> 6) % T, local id below R");
        CHECK(t.l2n[(size_t)owner * R + local] == v, "team: l2n[owner * R + local] == v");
        const uint64_t rw = t.rowl[(size_t)owner * R + local]; // k_push_team's pop: node 19 bits | degree 13 bits | first quad << 32
        CHECK(((uint32_t)rw & 0x7FFFFu) == v && ((uint32_t)(rw >> 19) & 8191u) == std::min(g.deg(v), 8191u) && (uint32_t)(rw >> 32) == t.rowq[v], "team: rowl packs (v, min(deg, 8191), rowq[v])");
        CHECK(t.deg16[(size_t)owner * R + local] == std::min(g.deg(v), 0xFFFFu), "team: deg16 is min(deg, 0xFFFF)");
    }
    CHECK(named == with_in, "team: l2n names the nodes with in-edges and nothing else");
    // hubs: the H largest by in-degree that have in-edges at all
    CHECK(t.H <= std::min<size_t>(hubs_opt, n) && (size_t)t.H * 8 + ((size_t)R + 1) * 8 + 23 * 1024 <= 163840 / TEAM_WGS_PER_CU, "team: hubs within the option, n and the LDS share");
    CHECK(t.hubtgt.size() == std::max(1u, t.H), "team: hubtgt has one entry at least");
    const std::vector<uint32_t> top = top_reference(indeg, t.H);
    std::vector<uint32_t> hub_of(n, TEAM_EMPTY);
    std::vector<uint64_t> hubs_owned(T, 0);
    for (uint32_t h = 0; h < t.H; h++) {
        if (!indeg[top[h]]) continue;
        hub_of[top[h]] = h;
        CHECK(t.hubtgt[h] == t.n2l[top[h]], "team: hubtgt[h] is the local name of the h-th node by (in-degree descending, id ascending)");
        hubs_owned[t.n2l[top[h]] >> TEAM_LBITS]++;
    }
    CHECK(t.colt.size() == (size_t)t.rowq[n] * 4, "team: colt is the quads of all rows");
    std::vector<uint64_t> edges((size_t)T * T, 0);
    for (size_t v = 0; v < n; v++) {
        const uint32_t *row = t.colt.data() + (size_t)t.rowq[v] * 4; // rows start at rowq[v] * 4
        const uint32_t d = g.deg(v);
        for (uint32_t k = 0; k < (d + 3) / 4 * 4; k++) {
            if (k >= d) { CHECK(row[k] == TEAM_EMPTY, "team: colt holds TEAM_EMPTY in a row's padding"); continue; }
            const uint32_t tg = (uint32_t)g.col[(size_t)g.row_ptr[v] + k];
            CHECK(row[k] == (hub_of[tg] != TEAM_EMPTY ? 0x80000000u | hub_of[tg] : t.n2l[tg]), "team: colt holds 0x80000000 | h for a hub target, n2l[target] otherwise");
            if (hub_of[tg] == TEAM_EMPTY) edges[((v >> 6) % T) * T + (t.n2l[tg] >> TEAM_LBITS)]++;
        }
    }
    CHECK(t.off.size() == (size_t)T * T + 1 && t.off[0] == 0, "team: off has T * T + 1 entries from 0");
    for (uint32_t s = 0; s < T; s++)
        for (uint32_t d = 0; d < T; d++) {
            const size_t i = (size_t)s * T + d;
            CHECK(t.off[i + 1] >= t.off[i] && (t.off[i + 1] - t.off[i]) % 16 == 0, "team: off ascends in whole 16-word steps");
            CHECK(t.off[i + 1] - t.off[i] >= 1 + edges[i] + hubs_owned[d], "team: bucket (s -> d) holds 1 + its edges to non-hub targets + the hubs d owns");
        }
    CHECK(t.cap == t.off[(size_t)T * T], "team: cap == off[T * T]");
    std::printf("team_R=%u team_H=%u ", t.R, t.H);
}

int main(int argc, char **argv) {
    if (argc != 9 && argc != 10) { std::printf("usage: %s <csr file> <shift> <pbins> <team force> <team max members> <team hubs> <push hubs> <dg_hubs> [tables]\n", argv[0]); return 2; }
    const auto on = [&](const char *table) { return argc == 9 || std::strstr(argv[9], table); };
    const Csr g = read_csr(argv[1]);
    const int shift = std::atoi(argv[2]), pbins = std::atoi(argv[3]);
    CHECK(shift >= 1 && shift <= 20 && pbins >= 0, "arguments: shift 1 .. 20, pbins >= 0");
    if (on("rows")) check_rows(g);
    if (on("compact")) check_compact(g);
    if (on("dg")) check_walk_dg(g, std::atoll(argv[8]));
    if (on("hubs")) check_hubs(g, (size_t)std::atoll(argv[7]), shift);
    if (on("quads")) check_quads(g);
    if (on("split")) check_split(g, shift, pbins);
    if (on("team")) check_team(g, (uint32_t)std::atoi(argv[4]), (uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
    std::printf("ok\n");
    return 0;
}
