// rows_check.cpp -- fora_amd/csrc/fora_rows.h on the CPU, against the contract restated by brute force: a dangling row is
// one entry, a live row is its held length, row_ptr is the prefix sum in the caller's order.  Stand-alone
// (tests/test_rows_cpu.py compiles it with the address and undefined-behaviour sanitizers):
//
//   rows_check layout <max_size> <rows> <batches>   rows: comma list, "d<source>" a dangling row, "<support>" a live one,
//                                                    "-" none; a leading "*": sources == nullptr (every row live, placed as
//                                                    row r0 + i); batches: comma list of live rows per batch, "-" none
//   rows_check geometry <tile>                       0: the kernels' SP_TILE
//   rows_check growth
//   rows_check threshold <value> ...                 prints the word of each value, or "rejected"
//
// Exit status 0 and one line of facts ("key=value ... ok"), or 1 and one line that names the first property that does not hold.
#include "fora_rows.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace fora;

[[noreturn]] static void failed(const char *what, const char *cond, int line) {
    std::printf("\nFAILED: %s [%s, line %d]\n", what, cond, line);
    std::exit(1);
}
#define CHECK(cond, what) do { if (!(cond)) failed(what, #cond, __LINE__); } while (0)

static std::vector<std::string> split(const char *list) {
    std::vector<std::string> out;
    if (!strcmp(list, "-")) return out;
    for (const char *p = list;;) {
        const char *q = strchr(p, ',');
        out.emplace_back(p, q ? (size_t)(q - p) : strlen(p));
        if (!q) return out;
        p = q + 1;
    }
}

static int check_layout(int64_t max_size, const char *rows_arg, const char *batches_arg) {
    const bool no_sources = rows_arg[0] == '*';
    const std::vector<std::string> rows = split(rows_arg + (no_sources ? 1 : 0));
    const int nq = (int)rows.size();
    std::vector<int32_t> sources((size_t)nq, 7);      // (a live row's source is never read)
    std::vector<bool> dangling((size_t)nq, false);
    std::vector<uint64_t> support((size_t)nq, 1), held((size_t)nq, 1);
    std::vector<int> live;
    for (int i = 0; i < nq; i++) {
        if (rows[(size_t)i][0] == 'd') {
            CHECK(!no_sources, "without sources there is no dangling row");
            dangling[(size_t)i] = true;
            sources[(size_t)i] = (int32_t)atoi(rows[(size_t)i].c_str() + 1);
            continue;
        }
        support[(size_t)i] = strtoull(rows[(size_t)i].c_str(), nullptr, 10);
        held[(size_t)i] = max_size > 0 ? std::min<uint64_t>(support[(size_t)i], (uint64_t)max_size) : support[(size_t)i];
        live.push_back(i);
    }
    // the contract, by brute force
    std::vector<int64_t> want_ptr((size_t)nq + 1, 0);
    for (int i = 0; i < nq; i++) want_ptr[(size_t)i + 1] = want_ptr[(size_t)i] + (int64_t)held[(size_t)i];
    uint64_t want_max = 0, want_support = 0;
    std::vector<int64_t> want_at;
    std::vector<int32_t> want_src;
    for (int i = 0; i < nq; i++) {
        want_max = std::max(want_max, support[(size_t)i]);
        want_support += support[(size_t)i];
        if (dangling[(size_t)i]) { want_at.push_back(want_ptr[(size_t)i]); want_src.push_back(sources[(size_t)i]); }
    }

    RowLayout lay;
    lay.max_row = 99; lay.cur = 99; lay.batches = 99; lay.dang_at.push_back(99); // (begin starts from nothing)
    lay.begin(no_sources ? nullptr : sources.data(), nq);
    CHECK(lay.row_ptr.size() == (size_t)nq + 1 && lay.cur == 0 && lay.written == 0 && lay.batches == 0 && lay.next_row == 0 && lay.dang_at.empty(), "begin");
    size_t at = 0;
    int nbatch = 0;
    uint64_t want_written = 0; // the end of the last live row of the batches before this one
    for (const std::string &b : split(batches_arg)) {
        const size_t nb = (size_t)atoi(b.c_str());
        CHECK(nb >= 1 && at + nb <= live.size(), "the batches hold the live rows");
        lay.begin_batch();
        nbatch++;
        for (size_t i = 0; i < nb; i++, at++) {
            const int row = live[at];
            CHECK(lay.written == want_written, "entries written before a place");
            CHECK(lay.written <= lay.cur, "nothing is written that is not placed");
            const int64_t base = lay.place(row, support[(size_t)row], held[(size_t)row]);
            CHECK(base == want_ptr[(size_t)row], "base of a live row");
            CHECK(lay.cur == (uint64_t)want_ptr[(size_t)row + 1] && lay.next_row == row + 1, "entries placed after a live row");
            CHECK(lay.batches == nbatch, "batches");
        }
        want_written = (uint64_t)want_ptr[(size_t)live[at - 1] + 1];
    }
    CHECK(at == live.size(), "every live row is in a batch");
    lay.finish();
    CHECK(lay.written == want_written && lay.written <= lay.cur, "entries written before the finish");
    CHECK(lay.row_ptr == want_ptr, "row_ptr is the prefix sum of the held lengths in the caller's order");
    CHECK(lay.dang_at == want_at && lay.dang_src == want_src, "the dangling list: entry and source of every dangling row, in order");
    CHECK(lay.cur == (uint64_t)want_ptr[(size_t)nq] && lay.max_row == want_max && lay.support == want_support, "cur, max_row, support");
    CHECK(lay.batches == nbatch && lay.next_row == nq && lay.nq == nq, "batches, next_row");
    std::printf("cur=%llu max_row=%llu support=%llu batches=%d dangling=%zu written=%llu row_ptr=", (unsigned long long)lay.cur, (unsigned long long)lay.max_row,
                (unsigned long long)lay.support, lay.batches, lay.dang_at.size(), (unsigned long long)lay.written);
    for (int i = 0; i <= nq; i++) std::printf("%s%lld", i ? "," : "", (long long)lay.row_ptr[(size_t)i]);
    std::printf(" ok\n");
    return 0;
}

static int check_geometry(uint64_t tile_arg) { // 0: the kernels' tile, through compact_geom's default argument
    const uint64_t tile = tile_arg ? tile_arg : (uint64_t)fora::SP_TILE;
    const uint64_t SP_TILE = tile; // (the name the expressions below were written with)
    int cases = 0;
    for (uint64_t n : {(uint64_t)1, (uint64_t)2, tile - 1, tile + 1, 8 * tile - 1, 8 * tile + 1, 1024 * 8 * tile - 1, 1024 * 8 * tile + 1, (uint64_t)0x7FFFFFFF}) {
        const CompactGeom g = tile_arg ? compact_geom(n, (uint32_t)tile) : compact_geom(n);
        const uint64_t R = g.R, X = g.X;
        CHECK(R % tile == 0 && R >= 8 * tile, "R: whole tiles, at least eight");
        CHECK(X >= 1 && X * R >= n && n > (X - 1) * R, "X workgroups of R ids cover n, and none is idle");
        CHECK(X <= 1024, "at most 1024 workgroups per slot"); // (R >= ceil(n / 1024), so for every n)
        // the expressions of sparse_prepare / sweep_prepare before there was a function
        const uint32_t R0 = (uint32_t)std::max<uint64_t>(8 * SP_TILE, ((n + 1023) / 1024 + SP_TILE - 1) / SP_TILE * SP_TILE);
        const uint32_t X0 = (uint32_t)((n + R0 - 1) / R0);
        CHECK(g.R == R0 && g.X == X0, "the geometry both prepare functions spelt out");
        cases++;
    }
    std::printf("cases=%d ok\n", cases);
    return 0;
}

static int check_growth() {
    int cases = 0;
    for (uint64_t rows_all : {(uint64_t)1, (uint64_t)2, (uint64_t)6, (uint64_t)1000, (uint64_t)0x7FFFFFFF})
        for (uint64_t rows_done : {(uint64_t)0, (uint64_t)1, rows_all})
            for (int sh = -1; sh <= 40; sh++)
                for (int64_t d = -1; d <= 1; d++) {
                    if (sh < 0 && d) continue;
                    const uint64_t need = sh < 0 ? 0 : (uint64_t)((int64_t)(1ull << sh) + d); // 0, and 2^sh - 1, 2^sh, 2^sh + 1 up to 2^40 + 1
                    const uint64_t cap = grow_guess(need, rows_done, rows_all);
                    CHECK(cap >= need && cap >= 1, "room for what is needed, and never an empty array");
                    // the expressions of sparse_reserve / sweep_reserve before there was a function
                    const uint64_t guess = rows_done ? (uint64_t)((double)need / (double)rows_done * (double)rows_all * 1.125) + 1024 : need;
                    const uint64_t cap0 = std::max<uint64_t>({need, guess, 1});
                    CHECK(cap == cap0, "the guess both reserve functions spelt out");
                    if (!rows_done) CHECK(cap == std::max<uint64_t>(need, 1), "no row placed: exactly what is needed");
                    cases++;
                }
    std::printf("cases=%d ok\n", cases);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "layout")) return check_layout(atoll(argv[2]), argv[3], argv[4]);
    if (argc == 3 && !strcmp(argv[1], "geometry")) return check_geometry(strtoull(argv[2], nullptr, 10));
    if (argc == 2 && !strcmp(argv[1], "growth")) return check_growth();
    if (argc >= 3 && !strcmp(argv[1], "threshold")) {
        for (int i = 2; i < argc; i++) {
            const double t = strtod(argv[i], nullptr); // (hex floats and "nan" too)
            if (threshold_ok(t)) std::printf("%llu\n", (unsigned long long)threshold_word(t));
            else std::printf("rejected\n");
        }
        return 0;
    }
    std::printf("usage: rows_check layout <max_size> <rows> <batches> | geometry <tile> | growth | threshold <value> ...\n");
    return 2;
}
