// subgraph_prop_plan_check.cpp -- the host side of SUBGRAPH PRODUCTS (fora_amd/csrc/fora_subgraph_prop_plan.h) against brute
// force, without a GPU.  Built with -fsanitize=address,undefined by tests/test_subgraph_prop_cpu.py and run directly.
//
//   subgraph_prop_plan_check cap <option>                          sub_short_cap of the option
//   subgraph_prop_plan_check csr <sub_short> <prop_segs> <ptr> <col|->   a square CSR in local ids: the split of its rows and of
//                                                             its columns into the one-pass kernel's and the long path's, the
//                                                             long path's plan, and the transposition, each held to brute
//                                                             force; prints "short=<r> long=<r> segs=<s> chunks=<c> t_short=<c>
//                                                             t_long=<c> t_segs=<s> ok", then in_ptr, in_row and in_pos, a line
//                                                             each ("-": empty)
//   subgraph_prop_plan_check all <sub_short> <prop_segs>      the same over built-in cases: rows and columns of 0, 1, 63, 64, 65,
//                                                             255, 256, 257, 300 and 700 edges with a duplicate edge, a
//                                                             self-loop, empty leading and trailing rows; no rows at all; rows
//                                                             without edges; one row of one self-loop; prints "cases=<n> ok"
#include "fora_subgraph_prop_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace fora;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static std::vector<int64_t> parse_list(const char *s) {
    std::vector<int64_t> out;
    if (!strcmp(s, "-")) return out;
    for (const char *p = s; *p;) {
        char *e;
        out.push_back(strtoll(p, &e, 10));
        p = *e ? e + 1 : e;
    }
    return out;
}

struct Csr { std::vector<int64_t> ptr; std::vector<int32_t> col; int rows() const { return (int)ptr.size() - 1; } };
struct Side { uint64_t short_rows = 0, long_rows = 0, segs = 0, chunks = 0; };

// the split and the long plan of one side against a row-by-row restatement; every array is sized exactly
static int check_side(const std::vector<int64_t> &ptr, int64_t option, uint64_t prop_segs, Side &out) {
    const int rows = (int)ptr.size() - 1;
    const uint32_t cap = sub_short_cap(option);
    CHECK(cap <= PROP_SEG);
    const SubSplit sp = sub_split(ptr.data(), rows, cap);
    const PropPlan plan = sub_long_plan(ptr.data(), rows, cap, prop_segs);
    const uint64_t per = std::max<uint64_t>(prop_segs, 1);
    uint64_t n_short = 0, n_long = 0, n_segs = 0, max_row = 0;
    std::vector<uint64_t> covered((size_t)rows, 0), finished((size_t)rows, 0);
    for (int i = 0; i < rows; i++) {
        const uint64_t len = (uint64_t)(ptr[(size_t)i + 1] - ptr[(size_t)i]);
        max_row = std::max(max_row, len);
        if (len <= cap) { n_short++; CHECK(sub_row_short(len, cap)); }
        else { n_long++; n_segs += (len + PROP_SEG - 1) / PROP_SEG; CHECK(!sub_row_short(len, cap)); CHECK(len > 0); }
    }
    CHECK(sp.short_rows == n_short && sp.long_rows == n_long && sp.long_segs == n_segs && sp.max_row == max_row);
    CHECK(plan.segs.size() == n_segs);
    CHECK(rows <= 0 ? plan.chunks.empty() : plan.chunks.size() == std::max<uint64_t>(1, (n_segs + per - 1) / per));
    // the segments: in row order, a long row's entries tiled from its first one in pieces of PROP_SEG
    size_t at = 0;
    for (int i = 0; i < rows; i++) {
        const uint64_t len = (uint64_t)(ptr[(size_t)i + 1] - ptr[(size_t)i]);
        if (len <= cap) continue;
        for (uint64_t o = 0; o < len; o += PROP_SEG, at++) {
            CHECK(at < plan.segs.size());
            const PropSeg &s = plan.segs[at];
            CHECK(s.row == i && s.first == ptr[(size_t)i] + (int64_t)o && s.len == std::min<uint64_t>(PROP_SEG, len - o));
        }
    }
    CHECK(at == plan.segs.size());
    // the chunks and records: a chunk's slots count up from 0, a record's slots are its row's next segments, a row is
    // finished by exactly one record and only long rows have records
    uint64_t seg0 = 0, rec0 = 0;
    for (const PropChunk &ch : plan.chunks) {
        CHECK(ch.seg0 == seg0 && ch.rec0 == rec0 && ch.nseg <= per);
        CHECK(ch.seg0 + ch.nseg <= plan.segs.size() && ch.rec0 + ch.nrec <= plan.recs.size());
        for (uint64_t k = 0; k < ch.nseg; k++) CHECK(plan.segs[(size_t)(seg0 + k)].slot == k);
        uint64_t slot = 0;
        for (uint64_t r = 0; r < ch.nrec; r++) {
            const PropRowRec &rec = plan.recs[(size_t)(rec0 + r)];
            CHECK(rec.row >= 0 && rec.row < rows);
            const uint64_t len = (uint64_t)(ptr[(size_t)rec.row + 1] - ptr[(size_t)rec.row]);
            CHECK(len > cap && rec.nseg >= 1 && rec.slot0 == slot && slot + rec.nseg <= ch.nseg);
            for (uint32_t k = 0; k < rec.nseg; k++) CHECK(plan.segs[(size_t)(seg0 + slot + k)].row == rec.row);
            CHECK(((rec.flags & PROP_FIRST) != 0) == (covered[(size_t)rec.row] == 0));
            covered[(size_t)rec.row] += rec.nseg;
            const bool last = covered[(size_t)rec.row] == (len + PROP_SEG - 1) / PROP_SEG;
            CHECK(((rec.flags & PROP_LAST) != 0) == last);
            finished[(size_t)rec.row] += last;
            slot += rec.nseg;
        }
        CHECK(slot == ch.nseg);
        seg0 += ch.nseg; rec0 += ch.nrec;
    }
    CHECK(seg0 == plan.segs.size() && rec0 == plan.recs.size());
    for (int i = 0; i < rows; i++) {
        const uint64_t len = (uint64_t)(ptr[(size_t)i + 1] - ptr[(size_t)i]);
        CHECK(finished[(size_t)i] == (len > cap ? 1u : 0u)); // every output row has one owner: k_sub_agg, or one combine record
    }
    out.short_rows = n_short; out.long_rows = n_long; out.segs = n_segs; out.chunks = plan.chunks.size();
    return 0;
}

struct Transposed { std::vector<int64_t> in_ptr, in_pos; std::vector<int32_t> in_row; };

static int check_transpose(const Csr &g, Transposed &t) {
    const int rows = g.rows();
    CHECK(sub_transpose_host(g.ptr.data(), g.col.data(), rows, t.in_ptr, t.in_row, t.in_pos));
    const size_t edges = g.col.size();
    CHECK(t.in_ptr.size() == (size_t)rows + 1 && t.in_row.size() == edges && t.in_pos.size() == edges);
    CHECK(t.in_ptr[0] == 0 && t.in_ptr[(size_t)rows] == (int64_t)edges);
    std::vector<int32_t> row_of(edges);
    for (int i = 0; i < rows; i++)
        for (int64_t e = g.ptr[(size_t)i]; e < g.ptr[(size_t)i + 1]; e++) row_of[(size_t)e] = i;
    for (int v = 0; v < rows; v++) { // brute force: the places whose target is v, ascending
        std::vector<int64_t> want;
        for (size_t e = 0; e < edges; e++) if (g.col[e] == v) want.push_back((int64_t)e);
        const int64_t lo = t.in_ptr[(size_t)v], hi = t.in_ptr[(size_t)v + 1];
        CHECK((size_t)(hi - lo) == want.size());
        // the device's way: the column's keys in whatever order the atomics left them (here: reversed), sorted
        std::vector<uint64_t> keys;
        for (size_t k = want.size(); k-- > 0;) {
            const int32_t i = row_of[(size_t)want[k]];
            keys.push_back(sub_key((uint32_t)i, (uint64_t)(want[k] - g.ptr[(size_t)i])));
        }
        std::sort(keys.begin(), keys.end());
        for (size_t k = 0; k < want.size(); k++) {
            CHECK(t.in_pos[(size_t)lo + k] == want[k] && t.in_row[(size_t)lo + k] == row_of[(size_t)want[k]]);
            const uint32_t i = (uint32_t)(keys[k] >> 32);
            CHECK((int32_t)i == t.in_row[(size_t)lo + k] && g.ptr[i] + (int64_t)(keys[k] & 0xFFFFFFFFull) == want[k]);
        }
    }
    return 0;
}

static int check_csr(const Csr &g, int64_t option, uint64_t prop_segs, Side &fwd, Side &tr, Transposed &t) {
    const int rows = g.rows();
    CHECK(rows >= 0 && g.ptr[0] == 0 && g.ptr[(size_t)rows] == (int64_t)g.col.size());
    for (int i = 0; i < rows; i++) CHECK(g.ptr[(size_t)i + 1] >= g.ptr[(size_t)i]);
    if (check_side(g.ptr, option, prop_segs, fwd)) return 1;
    if (check_transpose(g, t)) return 1;
    return check_side(t.in_ptr, option, prop_segs, tr);
}

static void print_list(const char *fmt, size_t n, const void *p, int width) {
    if (!n) { printf("-\n"); return; }
    for (size_t i = 0; i < n; i++) {
        if (width == 8) printf(fmt, (long long)((const int64_t *)p)[i]); else printf(fmt, (long long)((const int32_t *)p)[i]);
        putchar(i + 1 < n ? ',' : '\n');
    }
}

// rows H_k and columns C_k of LENS[k] edges each, through 700 filler nodes; a duplicate edge, a self-loop, empty ends
static Csr crafted() {
    static const int LENS[10] = {0, 1, 63, 64, 65, 255, 256, 257, 300, 700};
    const int H = 1, C = 11, F = 21, NF = 700, rows = F + NF + 1;
    std::vector<std::vector<int32_t>> adj((size_t)rows);
    for (int k = 0; k < 10; k++)
        for (int j = 0; j < LENS[k]; j++) adj[(size_t)(H + k)].push_back(F + j);
    adj[(size_t)(H + 2)][1] = adj[(size_t)(H + 2)][0];             // a duplicate edge: row H_2 keeps its 63 entries
    for (int j = 0; j < NF; j++)
        for (int k = 0; k < 10; k++)
            if (j < LENS[k]) adj[(size_t)(F + j)].push_back(C + k);
    adj[(size_t)F].push_back(F);                                      // a self-loop
    Csr g;
    g.ptr.push_back(0);
    for (const auto &a : adj) { g.col.insert(g.col.end(), a.begin(), a.end()); g.ptr.push_back((int64_t)g.col.size()); }
    return g;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "cap")) { printf("%u\n", sub_short_cap(strtoll(argv[2], nullptr, 10))); return 0; }
    if (argc == 6 && !strcmp(argv[1], "csr")) {
        Csr g;
        g.ptr = parse_list(argv[4]);
        for (int64_t v : parse_list(argv[5])) g.col.push_back((int32_t)v);
        CHECK(!g.ptr.empty());
        Side f, r; Transposed t;
        if (check_csr(g, strtoll(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), f, r, t)) return 1;
        printf("short=%llu long=%llu segs=%llu chunks=%llu t_short=%llu t_long=%llu t_segs=%llu ok\n", (unsigned long long)f.short_rows, (unsigned long long)f.long_rows,
               (unsigned long long)f.segs, (unsigned long long)f.chunks, (unsigned long long)r.short_rows, (unsigned long long)r.long_rows, (unsigned long long)r.segs);
        print_list("%lld", t.in_ptr.size(), t.in_ptr.data(), 8);
        print_list("%lld", t.in_row.size(), t.in_row.data(), 4);
        print_list("%lld", t.in_pos.size(), t.in_pos.data(), 8);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "all")) {
        const int64_t option = strtoll(argv[2], nullptr, 10);
        const uint64_t prop_segs = strtoull(argv[3], nullptr, 10);
        std::vector<Csr> cases;
        cases.push_back(crafted());
        cases.push_back(Csr{{0}, {}});                 // no rows at all
        cases.push_back(Csr{{0, 0, 0, 0}, {}});        // rows without edges
        cases.push_back(Csr{{0, 1}, {0}});             // one self-loop
        cases.push_back(Csr{{0, 3, 3, 5}, {1, 1, 0, 0, 2}}); // the four-node graph of the twin's rules over U = {0, 1, 3}
        int n = 0;
        for (const Csr &g : cases) {
            Side f, r; Transposed t;
            if (check_csr(g, option, prop_segs, f, r, t)) return 1;
            if (n == 0) { // the crafted lengths arrive on both sides
                const uint32_t cap = sub_short_cap(option);
                uint64_t want_long = 0;
                for (int len : {0, 1, 63, 64, 65, 255, 256, 257, 300, 700}) want_long += (uint32_t)len > cap;
                // (a filler node has at most 11 entries as a row and 10 as a column: short unless the cap is below that)
                CHECK(cap >= 11 ? f.long_rows == want_long && r.long_rows == want_long : f.long_rows >= want_long && r.long_rows >= want_long);
            }
            n++;
        }
        printf("cases=%d ok\n", n);
        return 0;
    }
    fprintf(stderr, "usage: subgraph_prop_plan_check cap <option> | csr <sub_short> <prop_segs> <ptr> <col|-> | all <sub_short> <prop_segs>\n");
    return 2;
}
