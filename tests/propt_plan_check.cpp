// propt_plan_check.cpp -- the host side of the transposition of PROPAGATE, TRANSPOSED (fora_amd/csrc/fora_propt_plan.h) against
// brute force, without a GPU.  Built with -fsanitize=address,undefined by tests/test_propagate_t_cpu.py and run directly.
//
//   propt_plan_check tiers <option> <len,len,...|->   the tier split of columns of these lengths; prints its facts
//   propt_plan_check network                          the sorting network of the lds and global tiers on runs of many lengths
#include "fora_propt_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>

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

static int check_tiers(int64_t option, const std::vector<int64_t> &lens) {
    const int64_t n = (int64_t)lens.size();
    std::vector<uint32_t> cnt(lens.begin(), lens.end());
    std::vector<int64_t> col_ptr((size_t)n + 1, -1);
    const uint64_t entries = propt_scan(cnt.data(), n, col_ptr.data());
    CHECK(col_ptr[0] == 0 && (uint64_t)col_ptr[(size_t)n] == entries);
    for (int64_t v = 0; v < n; v++) CHECK(col_ptr[(size_t)v + 1] - col_ptr[(size_t)v] == lens[(size_t)v]);
    const uint32_t cap = propt_lds_cap(option);
    CHECK(cap <= PROPT_LDS_MAX && (option < 0 ? cap == 0 : option > (int64_t)PROPT_LDS_MAX ? cap == PROPT_LDS_MAX : cap == (uint32_t)option));
    // brute force: every column, by the rule of the contract
    std::vector<PropTRun> want[4];
    uint64_t columns = 0, max_col = 0;
    uint32_t max_global = 0;
    for (int64_t v = 0; v < n; v++) {
        const uint64_t len = (uint64_t)lens[(size_t)v];
        columns += len > 0;
        max_col = std::max(max_col, len);
        int tier;
        if (len <= 1) tier = 0;
        else if (len > cap) tier = 3;
        else if (len <= 64) tier = 1;
        else tier = 2;
        CHECK(propt_tier(len, cap) == tier);
        if (tier == 3) max_global = std::max(max_global, (uint32_t)len);
        want[tier].push_back(PropTRun{col_ptr[(size_t)v], (uint32_t)len, 0});
    }
    const PropTTiers t = propt_tiers(col_ptr.data(), n, option);
    CHECK(t.n_short == want[1].size() && t.n_lds == want[2].size() && t.n_global == want[3].size());
    CHECK(t.runs.size() == (size_t)t.n_short + t.n_lds + t.n_global);
    CHECK(t.runs.size() <= propt_max_runs((uint64_t)n, entries));
    CHECK(t.columns == columns && t.max_col == max_col && t.max_global == max_global);
    size_t at = 0;
    for (int tier = 1; tier <= 3; tier++)
        for (const PropTRun &w : want[tier]) {
            const PropTRun &g = t.runs[at++];
            CHECK(g.first == w.first && g.len == w.len && g.pad_ == 0);
            CHECK(tier != 1 || g.len <= PROPT_SHORT);
            CHECK(tier != 2 || g.len <= PROPT_LDS_MAX);
        }
    printf("short=%u lds=%u global=%u columns=%llu max_col=%llu max_global=%u entries=%llu ok\n", t.n_short, t.n_lds, t.n_global,
           (unsigned long long)t.columns, (unsigned long long)t.max_col, t.max_global, (unsigned long long)entries);
    return 0;
}

// the network as the kernels run it: stage k = 2, 4, ... up to the power of two at or above len; a flip, then the strides
// k / 4 ... 1; P / 2 pairs per step; an exchange whose upper index is at or past len is skipped
static int check_network() {
    std::mt19937_64 rng(7300);
    std::vector<uint32_t> lens;
    for (uint32_t len = 1; len <= 140; len++) lens.push_back(len);
    for (uint32_t len : {255u, 256u, 257u, 511u, 513u, 600u, 1000u, 1023u, 1025u, 4095u, 4096u, 4097u, 5000u}) lens.push_back(len);
    for (uint32_t len : lens) {
        const uint32_t P = propt_pow2(len);
        CHECK(P >= len && (P & (P - 1)) == 0 && (P == 1 || P / 2 < len));
        for (int order = 0; order < 3; order++) { // shuffled, descending, ascending
            std::vector<uint64_t> key(len);
            for (uint32_t i = 0; i < len; i++) key[i] = ((uint64_t)(order == 1 ? len - 1 - i : i) << 32) | (rng() & 0xFFFFFFFFu);
            if (order == 0) std::shuffle(key.begin(), key.end(), rng);
            std::vector<uint64_t> want = key;
            std::sort(want.begin(), want.end());
            for (uint32_t k = 2; k <= P; k <<= 1)
                for (int step = 0;; step++) {
                    const uint32_t j = step == 0 ? 0 : (k >> 2) >> (step - 1);
                    if (step && !j) break;
                    std::vector<char> touched(P, 0);
                    for (uint32_t p = 0; p < P / 2; p++) {
                        const PropTPair pr = propt_pair(p, k, j);
                        CHECK(pr.lo < pr.hi && pr.hi < P);
                        CHECK(!touched[pr.lo] && !touched[pr.hi]); // the pairs of a step are disjoint: no order among them
                        touched[pr.lo] = touched[pr.hi] = 1;
                        if (pr.hi < len && key[pr.lo] > key[pr.hi]) std::swap(key[pr.lo], key[pr.hi]);
                    }
                }
            CHECK(key == want);
        }
    }
    printf("ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 4 && !strcmp(argv[1], "tiers")) return check_tiers(atoll(argv[2]), parse_list(argv[3]));
    if (argc >= 2 && !strcmp(argv[1], "network")) return check_network();
    printf("usage: propt_plan_check tiers <option> <lens> | network\n");
    return 2;
}
