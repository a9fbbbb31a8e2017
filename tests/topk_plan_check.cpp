// topk_plan_check.cpp -- the host side of the top-k sparse rows (fora_amd/csrc/fora_topk_plan.h) against brute force, without
// a GPU.  Built with -fsanitize=address,undefined by tests/test_sparse_topk_cpu.py and run directly.
//
//   topk_plan_check plan <k> <lds_cap option> <topk_cand option> <free entries> <n> <len,len,...|->
//       held lengths, tiers, chunks and stats of one batch of rows of these lengths; prints its facts
//   topk_plan_check clamp                                 the clamping of the two options
//   topk_plan_check wide                                  chunk bases and sums above 2^32
#include "fora_topk_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace fora;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static std::vector<uint32_t> parse_list(const char *s) {
    std::vector<uint32_t> out;
    if (!strcmp(s, "-")) return out;
    for (const char *p = s; *p;) {
        char *e;
        out.push_back((uint32_t)strtoull(p, &e, 10));
        p = *e ? e + 1 : e;
    }
    return out;
}

// the chunking by the rule of the contract, row by row: a row joins the open chunk while the chunk stays within cap; a row
// never splits, so a chunk always takes its first row
static int check_chunks(const std::vector<uint32_t> &len, uint64_t cap, const TopkBatchPlan &p) {
    const int nb = (int)len.size();
    CHECK(p.cand.size() == len.size());
    if (!nb) { CHECK(p.chunks.empty()); return 0; }
    CHECK(!p.chunks.empty() && p.chunks.front().r0 == 0 && p.chunks.back().r1 == nb);
    int row = 0;
    for (size_t j = 0; j < p.chunks.size(); j++) {
        const TopkChunk &c = p.chunks[j];
        CHECK(c.r0 == row && c.r1 > c.r0); // consecutive, none empty of rows
        uint64_t sum = 0;
        for (int i = c.r0; i < c.r1; i++) { CHECK(p.cand[(size_t)i] == sum); sum += len[(size_t)i]; }
        CHECK(sum == c.entries);
        CHECK(sum <= cap || c.r1 == c.r0 + 1);                           // over the cap: only a single row longer than it
        if (c.r1 < nb) CHECK(sum + len[(size_t)c.r1] > cap);              // greedy: the next row did not fit
        row = c.r1;
    }
    return 0;
}

static int cmd_plan(int64_t k, int64_t lds_opt, int64_t cand_opt, uint64_t free_entries, uint64_t n, const std::vector<uint32_t> &len) {
    CHECK(topk_k_ok(k));
    const uint32_t lds_cap = topk_lds_cap(lds_opt);
    uint64_t total = 0, longest = 0, held = 0, support = 0, max_support = 0;
    int cut = 0, lds = 0, glob = 0;
    TopkSums sums;
    for (const uint32_t l : len) {
        total += l; longest = std::max<uint64_t>(longest, l);
        const uint64_t h = topk_held(l, k);
        CHECK(h == ((uint64_t)l < (uint64_t)k ? l : (uint64_t)k));
        held += h;
        const TopkTier t = topk_tier(l, k, lds_cap);
        if ((uint64_t)l <= (uint64_t)k) CHECK(t == TOPK_COPY);
        else if (l <= lds_cap) { CHECK(t == TOPK_LDS); lds++; }
        else { CHECK(t == TOPK_GLOBAL); glob++; }
        cut += (uint64_t)l > (uint64_t)k;
        support += l; max_support = std::max<uint64_t>(max_support, l);
        sums.add_row(l, t);
    }
    CHECK(sums.support == support && sums.max_support == max_support && sums.cut_rows == cut && sums.lds_rows == lds && sums.global_rows == glob);
    CHECK(lds + glob == cut);
    const uint64_t cap = topk_cand_cap(cand_opt, free_entries, total, longest);
    CHECK(cap >= longest && cap >= 1);
    if (cand_opt > 0) CHECK(cap == std::max<uint64_t>({longest, std::min<uint64_t>(total, (uint64_t)cand_opt), 1}));
    else CHECK(cap == std::max<uint64_t>({longest, std::min<uint64_t>(total, free_entries), 1}));
    const TopkBatchPlan p = topk_chunks(len.data(), (int)len.size(), cap);
    if (check_chunks(len, cap, p)) return 1;
    for (const TopkChunk &c : p.chunks) {
        CHECK(c.entries <= cap); // (the cap holds the longest row: no chunk is over it)
        const int q0 = topk_launch_row(c.r0, n);
        CHECK(q0 == c.r0 || q0 == c.r0 - 1);
        CHECK(((uint64_t)q0 * n) % 2 == 0); // the launch's first row starts 16-byte aligned
        if (n % 2 == 0) CHECK(q0 == c.r0);
    }
    printf("held=%llu cut=%d lds=%d global=%d cap=%llu chunks=%zu first=", (unsigned long long)held, cut, lds, glob, (unsigned long long)cap, p.chunks.size());
    for (size_t j = 0; j < p.chunks.size(); j++) printf("%s%d", j ? "," : "", p.chunks[j].r0);
    printf("%s ok\n", p.chunks.empty() ? "-" : "");
    return 0;
}

static int cmd_clamp() {
    CHECK(topk_lds_cap(-5) == 0 && topk_lds_cap(0) == 0 && topk_lds_cap(1) == 1 && topk_lds_cap(64) == 64);
    CHECK(topk_lds_cap(TOPK_LDS_MAX) == TOPK_LDS_MAX && topk_lds_cap((int64_t)TOPK_LDS_MAX + 1) == TOPK_LDS_MAX && topk_lds_cap(INT64_MAX) == TOPK_LDS_MAX);
    CHECK((uint64_t)TOPK_LDS_MAX * 8 + 16384 <= 163840); // the staged words and 16 KiB beside them fit one CU's LDS
    CHECK(!topk_k_ok(0) && !topk_k_ok(-1) && !topk_k_ok(INT64_MIN) && topk_k_ok(1) && topk_k_ok(INT64_MAX));
    CHECK(topk_held(0, 1) == 0 && topk_held(5, INT64_MAX) == 5 && topk_held(UINT64_MAX, 7) == 7);
    // tiers at the cap and one beyond it
    for (const uint32_t cap : {0u, 1u, 64u, TOPK_LDS_MAX})
        for (const int64_t k : {(int64_t)1, (int64_t)63}) {
            CHECK(topk_tier((uint64_t)k, k, cap) == TOPK_COPY && topk_tier(0, k, cap) == TOPK_COPY);
            if ((uint64_t)cap > (uint64_t)k) CHECK(topk_tier(cap, k, cap) == TOPK_LDS);
            CHECK(topk_tier((uint64_t)cap + 1, k, cap) == ((uint64_t)cap + 1 <= (uint64_t)k ? TOPK_COPY : TOPK_GLOBAL));
            CHECK(topk_tier((uint64_t)k + 1, k, cap) == ((uint64_t)k + 1 <= cap ? TOPK_LDS : TOPK_GLOBAL));
        }
    CHECK(topk_cand_cap(-3, 100, 50, 10) == 50 && topk_cand_cap(0, 20, 50, 10) == 20 && topk_cand_cap(0, 5, 50, 10) == 10);
    CHECK(topk_cand_cap(1, 1000, 50, 10) == 10 && topk_cand_cap(30, 0, 50, 10) == 30 && topk_cand_cap(99, 0, 50, 10) == 50);
    CHECK(topk_cand_cap(0, 0, 0, 0) == 1);
    printf("ok\n");
    return 0;
}

static int cmd_wide() {
    // rows of 2^31 - 1 candidates: the bases inside a chunk and the sums pass 2^32
    const uint32_t big = 0x7FFFFFFFu;
    const std::vector<uint32_t> len{big, big, 7, big, 0, big, big};
    const uint64_t cap = 3ull * big + 7;
    const TopkBatchPlan p = topk_chunks(len.data(), (int)len.size(), cap);
    if (check_chunks(len, cap, p)) return 1;
    CHECK(p.chunks.size() == 2 && p.chunks[0].r1 == 5 && /* (the empty row rides with the full chunk) */p.chunks[0].entries == cap && p.cand[3] == 2ull * big + 7 && p.cand[3] > (1ull << 32));
    CHECK(p.chunks[1].entries == 2ull * big && p.cand[6] == big);
    TopkSums s;
    for (const uint32_t l : len) s.add_row(l, topk_tier(l, 64, TOPK_LDS_MAX));
    CHECK(s.support == 5ull * big + 7 && s.support > (1ull << 33) && s.max_support == big && s.cut_rows == 5 && s.global_rows == 5 && s.lds_rows == 0);
    const TopkRow r{p.cand[3], (1ull << 40) + 3, big, 64};
    CHECK(r.cand + r.len > (1ull << 32) && r.out > (1ull << 32));
    printf("ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 8 && !strcmp(argv[1], "plan"))
        return cmd_plan(strtoll(argv[2], nullptr, 10), strtoll(argv[3], nullptr, 10), strtoll(argv[4], nullptr, 10), strtoull(argv[5], nullptr, 10),
                        strtoull(argv[6], nullptr, 10), parse_list(argv[7]));
    if (argc == 2 && !strcmp(argv[1], "clamp")) return cmd_clamp();
    if (argc == 2 && !strcmp(argv[1], "wide")) return cmd_wide();
    printf("usage: topk_plan_check plan|clamp|wide ...\n");
    return 2;
}
