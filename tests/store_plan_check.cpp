// store_plan_check.cpp -- the host side of the ROW STORE (fora_amd/csrc/fora_store_plan.h) against brute force, without a GPU.
// Built with -fsanitize=address,undefined by tests/test_store_cpu.py and run directly.
//
//   store_plan_check take <span option> <store lens|-> <rows|->   the take plan of these indices over a store of rows of these
//                                                                 lengths; a bad index prints "rejected <place>"
//   store_plan_check rowptr <v,v,...>                             "ok" or "rejected": store_row_ptr_ok of the list
//   store_plan_check span <option>                                store_span of the option
#include "fora_store_plan.h"

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

static int take(int64_t option, const std::vector<int64_t> &lens, const std::vector<int64_t> &rows) {
    const int64_t R = (int64_t)lens.size(), nb = (int64_t)rows.size();
    std::vector<int64_t> store_ptr((size_t)R + 1, 0);
    for (int64_t i = 0; i < R; i++) store_ptr[(size_t)i + 1] = store_ptr[(size_t)i] + lens[(size_t)i];
    CHECK(store_row_ptr_ok(store_ptr.data(), R));
    const int64_t bad = store_bad_index(rows.data(), nb, R);
    int64_t want_bad = -1;
    for (int64_t i = nb - 1; i >= 0; i--) if (rows[(size_t)i] < 0 || rows[(size_t)i] >= R) want_bad = i;
    CHECK(bad == want_bad);
    if (bad >= 0) { printf("rejected %lld\n", (long long)bad); return 0; }
    const uint32_t span = store_span(option);
    CHECK(span >= 64 && span % 64 == 0 && span <= STORE_SPAN_MAX);
    const StorePlan p = store_take_plan(store_ptr.data(), rows.data(), nb, span);
    // brute force: the output, entry by entry, as (taken row, place in it)
    std::vector<int64_t> want_row, want_off;
    uint64_t max_row = 0;
    for (int64_t i = 0; i < nb; i++) {
        const int64_t len = lens[(size_t)rows[(size_t)i]];
        max_row = std::max<uint64_t>(max_row, (uint64_t)len);
        for (int64_t k = 0; k < len; k++) { want_row.push_back(i); want_off.push_back(k); }
    }
    const uint64_t E = want_row.size();
    CHECK(p.entries == E && p.max_row == max_row && p.span == span);
    CHECK(p.out_ptr.size() == (size_t)nb + 1 && p.src.size() == (size_t)nb && p.out_ptr[0] == 0 && (uint64_t)p.out_ptr[(size_t)nb] == E);
    for (int64_t i = 0; i < nb; i++) {
        CHECK(p.out_ptr[(size_t)i + 1] - p.out_ptr[(size_t)i] == lens[(size_t)rows[(size_t)i]]);
        CHECK(p.src[(size_t)i] == store_ptr[(size_t)rows[(size_t)i]]);
    }
    if (!E) { CHECK(p.spans == 0 && p.win.empty() && p.max_win == 0); printf("entries=0 spans=0 max_win=0 ok\n"); return 0; }
    CHECK(p.spans == (E + span - 1) / span && p.win.size() == (size_t)p.spans + 1 && p.win[(size_t)p.spans] == nb - 1);
    uint64_t max_win = 0;
    for (uint64_t s = 0; s < p.spans; s++) {
        // a span's window starts at the row of its first entry -- never an empty row -- and reaches the next span's
        CHECK(p.win[(size_t)s] == want_row[(size_t)(s * span)]);
        CHECK(p.win[(size_t)s + 1] >= p.win[(size_t)s]);
        max_win = std::max<uint64_t>(max_win, (uint64_t)(p.win[(size_t)s + 1] - p.win[(size_t)s]) + 1);
        const uint64_t e1 = std::min<uint64_t>((s + 1) * span, E);
        for (uint64_t e = s * span; e < e1; e++) { // what a lane does with entry e
            const int64_t r = store_find_row([&](int64_t i) { return p.out_ptr[(size_t)i]; }, p.win[(size_t)s], p.win[(size_t)s + 1], (int64_t)e);
            CHECK(r >= 0 && r < nb);
            CHECK(r == want_row[(size_t)e] && (int64_t)e - p.out_ptr[(size_t)r] == want_off[(size_t)e]);
            const int64_t from = p.src[(size_t)r] + ((int64_t)e - p.out_ptr[(size_t)r]);
            CHECK(from == store_ptr[(size_t)rows[(size_t)r]] + want_off[(size_t)e] && from < store_ptr[(size_t)R]);
        }
    }
    CHECK(p.max_win == max_win);
    printf("entries=%llu spans=%llu max_win=%llu ok\n", (unsigned long long)E, (unsigned long long)p.spans, (unsigned long long)p.max_win);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "take")) return take(atoll(argv[2]), parse_list(argv[3]), parse_list(argv[4]));
    if (argc == 3 && !strcmp(argv[1], "rowptr")) {
        const std::vector<int64_t> v = parse_list(argv[2]);
        CHECK(!v.empty());
        printf("%s\n", store_row_ptr_ok(v.data(), (int64_t)v.size() - 1) ? "ok" : "rejected");
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "span")) { printf("%u\n", store_span(atoll(argv[2]))); return 0; }
    fprintf(stderr, "usage: store_plan_check take <span> <lens> <rows> | rowptr <list> | span <option>\n");
    return 2;
}
