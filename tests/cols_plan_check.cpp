// cols_plan_check.cpp -- the arithmetic of COLUMNS (fora_amd/csrc/fora_cols_plan.h) against brute force, without a GPU.
// Built with -fsanitize=address,undefined by tests/test_cols_cpu.py and run directly.
//
//   cols_plan_check compact <n> <cols_block option> <ids|->   mark, totals, scan, list and relabel restated on the host through
//                                                             the header's functions, held to a sort-and-unique of the ids;
//                                                             prints "nc=<nc> words=<W> blocks=<B> ok"
//   cols_plan_check sets <n> <cols_block option>              the same over the id sets every n must survive: empty, a single id
//                                                             (each end), {0, n - 1}, every id, every 64th id, both sides of
//                                                             every word boundary; prints "sets=<count> ok"
//   cols_plan_check block <option>                            cols_block of the option
#include "fora_cols_plan.h"

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

struct Result { uint64_t nc = 0, words = 0, blocks = 0; };

// the five kernels' steps in their order, every array sized exactly (the sanitizer sees any index outside it)
static int compact(uint32_t n, int64_t option, const std::vector<int32_t> &ids, Result &res) {
    const uint64_t W = cols_words(n);
    const uint32_t block = cols_block(option);
    const uint64_t B = cols_blocks(W, block);
    CHECK(block >= COLS_BLOCK_MIN && block <= COLS_BLOCK_MAX && (block & (block - 1)) == 0);
    CHECK(W * 64 >= n && (W == 0 || (W - 1) * 64 < n));
    CHECK(B * block >= W && (B == 0 || (B - 1) * block < W));
    // mark
    std::vector<uint64_t> bitmap((size_t)W, 0);
    for (int32_t id : ids) {
        CHECK(id >= 0 && (uint32_t)id < n);
        bitmap[(size_t)cols_word_of((uint32_t)id)] |= cols_mask_of((uint32_t)id);
    }
    // totals
    std::vector<uint32_t> total((size_t)B, 0), off((size_t)B, 0);
    for (uint64_t b = 0; b < B; b++)
        for (uint64_t w = b * block; w < (b + 1) * block && w < W; w++) total[(size_t)b] += cols_popcount(bitmap[(size_t)w]);
    // scan
    uint64_t nc = 0;
    for (uint64_t b = 0; b < B; b++) { off[(size_t)b] = (uint32_t)nc; nc += total[(size_t)b]; }
    // list
    std::vector<uint32_t> wrank((size_t)W, 0);
    std::vector<int32_t> cols((size_t)nc, -1);
    for (uint64_t b = 0; b < B; b++) {
        uint32_t r = off[(size_t)b];
        for (uint64_t w = b * block; w < (b + 1) * block && w < W; w++) {
            wrank[(size_t)w] = r;
            for (uint64_t word = bitmap[(size_t)w]; word; word &= word - 1) {
                CHECK(r < nc);
                cols[(size_t)r++] = (int32_t)(w * 64 + (uint64_t)__builtin_ctzll(word));
            }
        }
        CHECK(r == off[(size_t)b] + total[(size_t)b]);
    }
    // relabel
    std::vector<int32_t> local(ids.size());
    for (size_t e = 0; e < ids.size(); e++) {
        const uint32_t id = (uint32_t)ids[e];
        const uint64_t w = cols_word_of(id);
        local[e] = (int32_t)cols_rank(wrank[(size_t)w], bitmap[(size_t)w], id & 63);
    }
    // ---- brute force: U by marking a byte per node, the rank by counting the marked nodes below
    std::vector<uint8_t> seen(n, 0);
    for (int32_t id : ids) seen[(size_t)id] = 1;
    std::vector<int32_t> want;
    std::vector<int32_t> rank_of(n, -1);
    for (uint32_t v = 0; v < n; v++)
        if (seen[v]) { rank_of[v] = (int32_t)want.size(); want.push_back((int32_t)v); }
    CHECK(nc == want.size());
    CHECK(cols == want);
    for (size_t e = 0; e < ids.size(); e++) {
        CHECK(local[e] == rank_of[(size_t)ids[e]]);
        CHECK(cols[(size_t)local[e]] == ids[e]);
    }
    for (size_t i = 1; i < cols.size(); i++) CHECK(cols[i - 1] < cols[i]);
    res.nc = nc; res.words = W; res.blocks = B;
    return 0;
}

static int sets(uint32_t n, int64_t option) {
    std::vector<std::vector<int32_t>> all;
    all.push_back({});
    all.push_back({0});
    all.push_back({(int32_t)n - 1});
    all.push_back({(int32_t)(n / 2)});
    all.push_back({0, (int32_t)n - 1});
    all.push_back({(int32_t)n - 1, 0, 0, (int32_t)n - 1}); // (any order, duplicates)
    std::vector<int32_t> every, every64, edges, down;
    for (uint32_t v = 0; v < n; v++) every.push_back((int32_t)v);
    for (uint32_t v = 0; v < n; v += 64) every64.push_back((int32_t)v);
    for (uint32_t v = 63; v < n; v += 64) { edges.push_back((int32_t)v); if (v + 1 < n) edges.push_back((int32_t)v + 1); }
    for (uint32_t v = n; v-- > 0;) down.push_back((int32_t)v);
    all.push_back(every); all.push_back(every64); all.push_back(edges); all.push_back(down);
    for (uint32_t v = 63; v < n; v += 64) { // both sides of each word boundary, one boundary at a time
        all.push_back({(int32_t)v});
        if (v + 1 < n) { all.push_back({(int32_t)v + 1}); all.push_back({(int32_t)v, (int32_t)v + 1}); }
    }
    for (const auto &ids : all) {
        Result r;
        if (compact(n, option, ids, r)) { printf("(n=%u, %zu ids, first %d)\n", n, ids.size(), ids.empty() ? -1 : ids[0]); return 1; }
    }
    printf("sets=%zu ok\n", all.size());
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "block")) {
        printf("%u\n", cols_block(strtoll(argv[2], nullptr, 10)));
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "sets")) return sets((uint32_t)strtoul(argv[2], nullptr, 10), strtoll(argv[3], nullptr, 10));
    if (argc == 5 && !strcmp(argv[1], "compact")) {
        const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 10);
        std::vector<int32_t> ids;
        for (int64_t v : parse_list(argv[4])) ids.push_back((int32_t)v);
        Result r;
        if (compact(n, strtoll(argv[3], nullptr, 10), ids, r)) return 1;
        printf("nc=%llu words=%llu blocks=%llu ok\n", (unsigned long long)r.nc, (unsigned long long)r.words, (unsigned long long)r.blocks);
        return 0;
    }
    fprintf(stderr, "usage: cols_plan_check compact <n> <block> <ids|-> | sets <n> <block> | block <option>\n");
    return 2;
}
