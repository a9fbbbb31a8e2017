// subgraph_plan_check.cpp -- the arithmetic of SUBGRAPH (fora_amd/csrc/fora_subgraph_plan.h) against brute force, without a GPU.
// Built with -fsanitize=address,undefined by tests/test_subgraph_cpu.py and run directly.
//
//   subgraph_plan_check graph <n> <sub_span option> <row_ptr> <col|-> <U|->   rows, count, scan and write restated on the host
//                                                             through the header's functions, held to a row-by-row filter;
//                                                             prints "edges=<E> scanned=<S> spans=<P> ok", then sub_ptr,
//                                                             sub_col and sub_eid, a line each ("-": empty)
//   subgraph_plan_check all <n> <sub_span option>             the same over the degree patterns (all 0; all 1; one row of 20
//                                                             spans among rows of 0 and 1; rows that end exactly on a span
//                                                             boundary; leading and trailing empty rows -- with self-loops and
//                                                             duplicate edges) times the sets U every n must survive: empty, a
//                                                             single node, {0, n - 1}, every node, both sides of every word
//                                                             boundary; prints "cases=<count> ok"
//   subgraph_plan_check span <option>                         sub_span of the option
#include "fora_subgraph_plan.h"

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

struct Graph { uint32_t n = 0; std::vector<int64_t> row_ptr; std::vector<int32_t> col; };
struct Result { uint64_t S = 0, spans = 0; std::vector<int64_t> sub_ptr, sub_eid; std::vector<int32_t> sub_col; };

// the kernels' steps in their order, every array sized exactly (the sanitizer sees any index outside it).  U: ascending, distinct
static int induce(const Graph &g, const std::vector<int32_t> &U, int64_t option, Result &res) {
    const uint32_t n = g.n, span = sub_span(option);
    const uint64_t nc = U.size(), nnz = g.col.size();
    CHECK(span >= SUB_SPAN_MIN && span <= SUB_SPAN_MAX && (span & (span - 1)) == 0);
    // the bitmap of U and the rank of every word's first set bit, as COLUMNS leaves them
    const uint64_t W = cols_words(n);
    std::vector<uint64_t> bitmap((size_t)W, 0);
    std::vector<uint32_t> wrank((size_t)W, 0);
    for (int32_t u : U) { CHECK(u >= 0 && (uint32_t)u < n); bitmap[(size_t)cols_word_of((uint32_t)u)] |= cols_mask_of((uint32_t)u); }
    for (uint64_t w = 0, r = 0; w < W; w++) { wrank[(size_t)w] = (uint32_t)r; r += cols_popcount(bitmap[(size_t)w]); }
    // rows
    std::vector<int64_t> scan_ptr((size_t)nc + 1, 0), base((size_t)nc, 0);
    for (uint64_t j = 0; j < nc; j++) {
        const int64_t first = g.row_ptr[(size_t)U[(size_t)j]], deg = g.row_ptr[(size_t)U[(size_t)j] + 1] - first;
        base[(size_t)j] = first - scan_ptr[(size_t)j];
        scan_ptr[(size_t)j + 1] = scan_ptr[(size_t)j] + deg;
    }
    const uint64_t S = (uint64_t)scan_ptr[(size_t)nc], P = sub_spans(S, span);
    CHECK(P * span >= S && (P == 0 || (P - 1) * span < S));
    const auto ptr = [&](int64_t i) { return scan_ptr.at((size_t)i); };
    struct Win { int64_t start, lo, hi; uint32_t len; };
    const auto window = [&](uint64_t s) {
        Win w;
        w.start = (int64_t)(s * span);
        w.len = (uint32_t)std::min<uint64_t>(span, S - (uint64_t)w.start);
        w.lo = sub_find_row(ptr, 0, (int64_t)nc - 1, w.start);
        w.hi = sub_find_row(ptr, w.lo, (int64_t)nc - 1, w.start + w.len - 1);
        return w;
    };
    // one scanned edge: its row inside the window, its place in col, its target, whether it is kept
    int bad = 0;
    const auto edge = [&](const Win &w, int64_t p, int64_t &e, uint32_t &t) {
        const int64_t r = sub_find_row(ptr, w.lo, w.hi, p);
        if (!(r >= w.lo && r <= w.hi && scan_ptr[(size_t)r] <= p && p < scan_ptr[(size_t)r + 1])) bad++;
        e = base.at((size_t)r) + p;
        if (!(e >= g.row_ptr[(size_t)U[(size_t)r]] && e < g.row_ptr[(size_t)U[(size_t)r] + 1] && (uint64_t)e < nnz)) { bad++; return false; }
        t = (uint32_t)g.col[(size_t)e];
        return t < n && sub_member(bitmap.at((size_t)cols_word_of(t)), t);
    };
    // count
    std::vector<uint32_t> cnt((size_t)P, 0);
    for (uint64_t s = 0; s < P; s++) {
        const Win w = window(s);
        CHECK(w.len >= 1 && w.len <= span && w.lo <= w.hi);
        for (uint32_t i = 0; i < w.len; i++) { int64_t e; uint32_t t; cnt[(size_t)s] += edge(w, w.start + i, e, t) ? 1 : 0; }
    }
    CHECK(!bad);
    // scan
    std::vector<uint64_t> off((size_t)P, 0);
    uint64_t edges = 0;
    for (uint64_t s = 0; s < P; s++) { off[(size_t)s] = edges; edges += cnt[(size_t)s]; }
    // write
    res.sub_ptr.assign((size_t)nc + 1, -1); res.sub_col.assign((size_t)edges, -1); res.sub_eid.assign((size_t)edges, -1);
    std::vector<int> written((size_t)nc + 1, 0);
    for (uint64_t s = 0; s < P; s++) {
        const Win w = window(s);
        std::vector<uint32_t> pref((size_t)w.len + 1, 0);
        uint32_t carry = 0;
        for (uint32_t i = 0; i < w.len; i++) {
            int64_t e = 0; uint32_t t = n;
            const bool keep = edge(w, w.start + i, e, t);
            pref[i] = carry;
            if (keep) {
                const uint64_t k = off[(size_t)s] + carry++;
                CHECK(k < edges && res.sub_col[(size_t)k] == -1);
                const uint64_t word = cols_word_of(t);
                res.sub_col[(size_t)k] = (int32_t)cols_rank(wrank[(size_t)word], bitmap[(size_t)word], t & 63);
                res.sub_eid[(size_t)k] = e;
            }
        }
        pref[w.len] = carry;
        CHECK(carry == cnt[(size_t)s]);
        const int64_t ja = sub_rows_from(ptr, (int64_t)nc, w.start);
        const int64_t jb = s + 1 == P ? (int64_t)nc + 1 : sub_rows_from(ptr, (int64_t)nc, w.start + w.len);
        CHECK(ja >= 0 && ja <= jb && jb <= (int64_t)nc + 1);
        for (int64_t j = ja; j < jb; j++) {
            const int64_t at = scan_ptr[(size_t)j] - w.start;
            CHECK(at >= 0 && at <= (int64_t)w.len);
            res.sub_ptr[(size_t)j] = (int64_t)(off[(size_t)s] + pref[(size_t)at]);
            written[(size_t)j]++;
        }
    }
    if (!P) for (auto &x : res.sub_ptr) x = 0; // (the driver clears sub_ptr when nothing is scanned)
    else for (uint64_t j = 0; j <= nc; j++) CHECK(written[(size_t)j] == 1);
    // ---- brute force: a byte per node, the rank by counting the members below, row by row
    std::vector<int32_t> rank_of(n, -1);
    for (size_t j = 0; j < U.size(); j++) { CHECK(j == 0 || U[j - 1] < U[j]); rank_of[(size_t)U[j]] = (int32_t)j; }
    std::vector<int64_t> want_ptr{0}, want_eid;
    std::vector<int32_t> want_col;
    for (int32_t u : U) {
        for (int64_t e = g.row_ptr[(size_t)u]; e < g.row_ptr[(size_t)u + 1]; e++)
            if (rank_of[(size_t)g.col[(size_t)e]] >= 0) { want_col.push_back(rank_of[(size_t)g.col[(size_t)e]]); want_eid.push_back(e); }
        want_ptr.push_back((int64_t)want_col.size());
    }
    CHECK(edges == want_col.size());
    CHECK(res.sub_ptr == want_ptr);
    CHECK(res.sub_col == want_col);
    CHECK(res.sub_eid == want_eid);
    res.S = S; res.spans = P;
    return 0;
}

// the degree patterns; targets from a small generator, a self-loop at the head of every third non-empty row, every fifth edge
// a copy of the one in front of it
static Graph pattern(uint32_t n, int kind, uint32_t span) {
    Graph g;
    g.n = n;
    g.row_ptr.push_back(0);
    uint64_t x = 0x9E3779B97F4A7C15ull ^ ((uint64_t)n << 8) ^ (uint64_t)kind;
    for (uint32_t v = 0; v < n; v++) {
        uint64_t deg = 0;
        switch (kind) {
            case 0: deg = 0; break;
            case 1: deg = 1; break;
            case 2: deg = v == n / 2 ? 20ull * span : v % 2; break;                        // a hub of 20 spans among rows of 0 and 1
            case 3: deg = v < 2 ? span : (v == 2 ? span - 3 : (v == 3 ? 3 : v % 3)); break;  // rows that end exactly on a span boundary
            default: deg = v < n / 3 || v >= n - n / 3 ? 0 : 2; break;                     // leading and trailing empty rows
        }
        for (uint64_t i = 0; i < deg; i++) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            int32_t t = (int32_t)((x >> 33) % n);
            if (i == 0 && v % 3 == 0) t = (int32_t)v;
            else if (i % 5 == 4) t = g.col.back();
            g.col.push_back(t);
        }
        g.row_ptr.push_back((int64_t)g.col.size());
    }
    return g;
}

static int all(uint32_t n, int64_t option) {
    std::vector<std::vector<int32_t>> sets;
    sets.push_back({});
    sets.push_back({0});
    sets.push_back({(int32_t)n - 1});
    sets.push_back({(int32_t)(n / 2)});
    if (n > 1) sets.push_back({0, (int32_t)n - 1});
    std::vector<int32_t> every, edges, odd;
    for (uint32_t v = 0; v < n; v++) every.push_back((int32_t)v);
    for (uint32_t v = 1; v < n; v += 2) odd.push_back((int32_t)v);
    for (uint32_t v = 63; v < n; v += 64) { edges.push_back((int32_t)v); if (v + 1 < n) edges.push_back((int32_t)v + 1); }
    sets.push_back(every); sets.push_back(odd); sets.push_back(edges);
    for (uint32_t v = 63; v < n; v += 64) { // both sides of each word boundary, one boundary at a time, beside the hub of pattern 2
        const int32_t hub = (int32_t)(n / 2);
        for (std::vector<int32_t> s : {std::vector<int32_t>{(int32_t)v}, std::vector<int32_t>{(int32_t)v + 1}, std::vector<int32_t>{(int32_t)v, (int32_t)v + 1}}) {
            if ((uint32_t)s.back() >= n) continue;
            if (hub != s[0] && hub != s.back()) s.insert(hub < s[0] ? s.begin() : s.end(), hub);
            sets.push_back(s);
        }
    }
    size_t cases = 0;
    const uint32_t span = sub_span(option);
    for (int kind = 0; kind < 5; kind++) {
        const Graph g = pattern(n, kind, span);
        for (const auto &U : sets) {
            Result r;
            if (induce(g, U, option, r)) { printf("(n=%u, pattern %d, %zu nodes, first %d)\n", n, kind, U.size(), U.empty() ? -1 : U[0]); return 1; }
            cases++;
        }
    }
    printf("cases=%zu ok\n", cases);
    return 0;
}

template <typename T> static void print_list(const std::vector<T> &v) {
    if (v.empty()) printf("-");
    for (size_t i = 0; i < v.size(); i++) printf("%s%lld", i ? "," : "", (long long)v[i]);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "span")) {
        printf("%u\n", sub_span(strtoll(argv[2], nullptr, 10)));
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "all")) return all((uint32_t)strtoul(argv[2], nullptr, 10), strtoll(argv[3], nullptr, 10));
    if (argc == 7 && !strcmp(argv[1], "graph")) {
        Graph g;
        g.n = (uint32_t)strtoul(argv[2], nullptr, 10);
        g.row_ptr = parse_list(argv[4]);
        for (int64_t v : parse_list(argv[5])) g.col.push_back((int32_t)v);
        std::vector<int32_t> U;
        for (int64_t v : parse_list(argv[6])) U.push_back((int32_t)v);
        CHECK(g.row_ptr.size() == (size_t)g.n + 1 && g.row_ptr[0] == 0 && (size_t)g.row_ptr.back() == g.col.size());
        for (int32_t t : g.col) CHECK(t >= 0 && (uint32_t)t < g.n);
        Result r;
        if (induce(g, U, strtoll(argv[3], nullptr, 10), r)) return 1;
        printf("edges=%zu scanned=%llu spans=%llu ok\n", r.sub_col.size(), (unsigned long long)r.S, (unsigned long long)r.spans);
        print_list(r.sub_ptr); print_list(r.sub_col); print_list(r.sub_eid);
        return 0;
    }
    fprintf(stderr, "usage: subgraph_plan_check graph <n> <span> <row_ptr> <col|-> <U|-> | all <n> <span> | span <option>\n");
    return 2;
}
