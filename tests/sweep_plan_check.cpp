// sweep_plan_check.cpp -- fora_amd/csrc/fora_sweep_plan.h on the CPU, against the plan of a sweep batch restated by brute
// force.  Stand-alone (tests/test_sweep_cpu.py compiles it with the address and undefined-behaviour sanitizers):
//
//   sweep_plan_check tile <option> ...                    the sort tile of each value of the option sweep_lds_cap
//   sweep_plan_check plan <T> <max_size> <rows> <batches> rows: comma list, "d<source>" a dangling row, "<support>" a live one;
//                                                         a leading "*": no sources, every row live and slot i of a batch row
//                                                         r0 + i (otherwise through `at`); batches: live rows per batch
//
// Exit status 0 and facts ("key=value ... ok"), or 1 and one line that names the first property that does not hold.
#include "fora_sweep_plan.h"

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

template <class T> static bool same_bytes(const T *got, const std::vector<T> &want) { // (got: inside a vector of words)
    return want.empty() || !memcmp(got, want.data(), want.size() * sizeof(T));
}

static int check_plan(uint32_t T, int64_t max_size, const char *rows_arg, const char *batches_arg) {
    const bool identity = rows_arg[0] == '*';
    const std::vector<std::string> rows = split(rows_arg + (identity ? 1 : 0));
    const int nq = (int)rows.size();
    std::vector<int32_t> sources((size_t)nq, 7);
    std::vector<uint32_t> support((size_t)nq, 0);
    std::vector<int> live;
    for (int i = 0; i < nq; i++) {
        if (rows[(size_t)i][0] == 'd') { CHECK(!identity, "without sources there is no dangling row"); continue; }
        support[(size_t)i] = (uint32_t)strtoul(rows[(size_t)i].c_str(), nullptr, 10);
        live.push_back(i);
    }
    RowLayout lay;
    lay.begin(identity ? nullptr : sources.data(), nq);
    struct Kept { int row; SweepRowDesc rd; };
    std::vector<Kept> kept;
    size_t done = 0, ntiles = 0, ngrows = 0;
    uint64_t words = 0;
    uint32_t maxP_all = 0;
    for (const std::string &b : split(batches_arg)) {
        const int nb = atoi(b.c_str());
        CHECK(nb >= 1 && done + (size_t)nb <= live.size(), "the batches hold the live rows");
        std::vector<uint32_t> h_tot((size_t)nb); // (exactly the batch's counts)
        std::vector<int> at((size_t)nb);
        for (int i = 0; i < nb; i++) { at[(size_t)i] = live[done + (size_t)i]; h_tot[(size_t)i] = support[(size_t)at[(size_t)i]]; }
        const int batches_before = lay.batches;
        const SweepBatchPlan p = sweep_batch_plan(h_tot.data(), nb, max_size, T, lay, identity ? nullptr : at.data(), identity ? (int)done : -1000);
        CHECK(lay.batches == batches_before + 1 && lay.next_row == at[(size_t)nb - 1] + 1, "one batch opened, its rows placed in slot order");
        CHECK(p.rd.size() == (size_t)nb && p.tbase.size() == (size_t)nb, "a descriptor and a base per slot");
        // every row; the tiles and global rows of the batch, in slot order
        std::vector<SweepTile> want_tiles;
        std::vector<SweepGRow> want_grows;
        uint64_t tneed = 0;
        uint32_t maxP = 0, maxL = 0;
        for (int i = 0; i < nb; i++) {
            const SweepRowDesc &rd = p.rd[(size_t)i];
            const uint32_t len = h_tot[(size_t)i];
            CHECK(rd.len == len && rd.pad_ == 0, "len");
            if (!len) CHECK(rd.P == 0, "an empty row has no padded copy");
            else CHECK((rd.P & (rd.P - 1)) == 0 && rd.P >= len && (rd.P == 1 || rd.P / 2 < len), "P: the least power of two that holds the row");
            CHECK(rd.L == (max_size > 0 ? (uint32_t)std::min<int64_t>(len, max_size) : len), "L: the support, cut at max_size");
            CHECK(rd.tbase == (int64_t)tneed && p.tbase[(size_t)i] == rd.tbase, "tbase: the prefix sum of P");
            if (T >= 2) {
                if (rd.P && rd.P < T) want_tiles.push_back(SweepTile{rd.tbase, rd.P, 0}); // a row shorter than a tile: one, at offset 0
                else for (uint64_t off = 0; off < rd.P; off += T) want_tiles.push_back(SweepTile{rd.tbase + (int64_t)off, rd.P, (uint32_t)off});
            }
            if (rd.P > T) want_grows.push_back(SweepGRow{rd.tbase, rd.P, 0});
            tneed += rd.P;
            maxP = std::max(maxP, rd.P); maxL = std::max(maxL, rd.L);
            kept.push_back(Kept{at[(size_t)i], rd});
        }
        CHECK(p.tneed == tneed && p.maxP == maxP && p.maxL == maxL, "tneed, maxP, maxL");
        CHECK(p.tiles.size() == want_tiles.size() && same_bytes(p.tiles.data(), want_tiles), "the tiles of a row tile [tbase, tbase + P) in steps of T; none for T == 1");
        for (const SweepTile &t : p.tiles) CHECK(t.off % T == 0 && t.off < t.P && t.base >= (int64_t)t.off && (uint64_t)t.base - t.off + t.P <= tneed, "a tile lies inside its row");
        CHECK(p.grows.size() == want_grows.size() && same_bytes(p.grows.data(), want_grows), "the global rows are the rows with P > T");
        // the upload, read back through the view from a vector of exactly the planned size
        const std::vector<uint64_t> copy(p.pack);
        const SweepDescView<const uint64_t> v = p.view<const uint64_t>(copy.data());
        CHECK(copy.size() == v.words() && v.words() == (size_t)nb * 5 + p.tiles.size() * 2 + p.grows.size() * 2, "words of the upload");
        CHECK(same_bytes(v.rows(), p.rd) && same_bytes(v.tbase(), p.tbase) && same_bytes(v.tiles(), p.tiles) && same_bytes(v.grows(), p.grows), "the four parts read back");
        CHECK((const void *)(v.grows() + p.grows.size()) == (const void *)(copy.data() + copy.size()), "the parts fill the words");
        done += (size_t)nb; ntiles += p.tiles.size(); ngrows += p.grows.size(); words += p.pack.size();
        maxP_all = std::max(maxP_all, p.maxP);
    }
    CHECK(done == live.size(), "every live row is in a batch");
    lay.finish();
    for (const Kept &k : kept) CHECK(k.rd.hbase == lay.row_ptr[(size_t)k.row], "hbase: the row's entry in the finished layout's row_ptr");
    for (const Kept &k : kept) CHECK(lay.row_ptr[(size_t)k.row + 1] - lay.row_ptr[(size_t)k.row] == (int64_t)k.rd.L, "the layout holds L entries of the row");
    std::printf("live=%zu tiles=%zu global_rows=%zu maxP=%u words=%llu entries=%llu ok\n", live.size(), ntiles, ngrows, maxP_all, (unsigned long long)words, (unsigned long long)lay.cur);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && !strcmp(argv[1], "tile")) {
        for (int i = 2; i < argc; i++) std::printf("%u\n", sweep_tile(atoll(argv[i])));
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "plan")) return check_plan((uint32_t)strtoul(argv[2], nullptr, 10), atoll(argv[3]), argv[4], argv[5]);
    std::printf("usage: sweep_plan_check tile <option> ... | plan <T> <max_size> <rows> <batches>\n");
    return 2;
}
