// softmax_plan_check.cpp -- the host side of ROW SOFTMAX (fora_amd/csrc/fora_softmax_plan.h) against brute force, without a
// GPU.  Built with -fsanitize=address,undefined by tests/test_softmax_cpu.py and run directly.
//
//   softmax_plan_check <option> <len,len,...|->   the two work lists of rows of these lengths under softmax_short = option
#include "fora_softmax_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

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

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: softmax_plan_check <option> <lens>\n"); return 2; }
    const int64_t option = atoll(argv[1]);
    const std::vector<int64_t> lens = parse_list(argv[2]);
    const int nq = (int)lens.size();
    std::vector<int64_t> row_ptr((size_t)nq + 1, 0);
    for (int i = 0; i < nq; i++) row_ptr[(size_t)i + 1] = row_ptr[(size_t)i] + lens[(size_t)i];
    const uint32_t cap = softmax_short_cap(option);
    CHECK(cap <= 256 && (option < 0 ? cap == 0 : option > 256 ? cap == 256 : cap == (uint32_t)option));
    const uint64_t total = prop_segments(row_ptr.data(), nq);
    const PropPlan plan = prop_plan(row_ptr.data(), nq, std::max<uint64_t>(total, 1));
    const SoftmaxLists l = softmax_lists(plan.segs, row_ptr.data(), cap);
    CHECK(l.n_short + l.n_long == total && l.segs.size() == total);
    // brute force: every entry of every row is covered once, by the list its row's length says, in row and entry order
    std::vector<int> covered((size_t)row_ptr[(size_t)nq], 0);
    uint64_t short_rows = 0, long_rows = 0;
    for (int i = 0; i < nq; i++) {
        if (lens[(size_t)i] && (uint64_t)lens[(size_t)i] <= cap) short_rows++;
        if ((uint64_t)lens[(size_t)i] > cap) long_rows++;
    }
    CHECK(l.short_rows == short_rows && l.long_rows == long_rows && l.n_short == short_rows);
    int64_t last_first = -1;
    for (uint64_t u = 0; u < l.n_short; u++) {
        const PropSeg &s = l.segs[(size_t)u];
        CHECK(s.row >= 0 && s.row < nq && s.first == row_ptr[(size_t)s.row] && (int64_t)s.len == lens[(size_t)s.row] && s.len >= 1 && s.len <= cap);
        CHECK(s.first > last_first);
        last_first = s.first;
        for (uint32_t k = 0; k < s.len; k++) covered[(size_t)(s.first + k)]++;
    }
    const PropSeg *lng = l.segs.data() + l.n_short;
    last_first = -1;
    for (uint64_t u = 0; u < l.n_long; u++) {
        const PropSeg &s = lng[u];
        CHECK(s.row >= 0 && s.row < nq && (uint64_t)lens[(size_t)s.row] > cap && s.len >= 1 && s.len <= PROP_SEG);
        CHECK(s.first > last_first);
        last_first = s.first;
        const uint64_t nseg = ((uint64_t)lens[(size_t)s.row] + PROP_SEG - 1) / PROP_SEG;
        CHECK(s.pad_ == nseg && (uint64_t)s.slot + nseg <= l.n_long && s.slot <= u && u < (uint64_t)s.slot + nseg);
        // the row's segments are the nseg of the list from slot on, consecutive cuts of the row
        const uint64_t k = u - s.slot;
        CHECK(lng[s.slot].row == s.row && lng[s.slot].first == row_ptr[(size_t)s.row]);
        CHECK(s.first == row_ptr[(size_t)s.row] + (int64_t)(k * PROP_SEG));
        CHECK(s.len == std::min<uint64_t>(PROP_SEG, (uint64_t)lens[(size_t)s.row] - k * PROP_SEG));
        for (uint32_t j = 0; j < s.len; j++) covered[(size_t)(s.first + j)]++;
    }
    for (int c : covered) CHECK(c == 1);
    printf("short=%llu long=%llu short_rows=%llu long_rows=%llu ok\n", (unsigned long long)l.n_short, (unsigned long long)l.n_long,
           (unsigned long long)l.short_rows, (unsigned long long)l.long_rows);
    return 0;
}
