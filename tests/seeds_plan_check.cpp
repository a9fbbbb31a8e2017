// seeds_plan_check.cpp -- fora_amd/csrc/fora_seeds_plan.h on the CPU, against the SEED SETS rules restated by brute force.
// Stand-alone (tests/test_seeds_plan_cpu.py compiles it with the address and undefined-behaviour sanitizers):
//
//   seeds_plan_check sets <ns> <set_ptr> <seeds>       comma lists, "null" a null pointer; prints the refusal or "fine"
//   seeds_plan_check uniform <k>                       the words of one set of k seeds without weights, one per line
//   seeds_plan_check weights <value> ...               the words of one set with these weights (hex floats), or "refused: <text>"
//   seeds_plan_check plan <dedup> <per> <row_ptr> <sets>
//                                                      row_ptr: comma list of the graph's; sets: seeds by comma, sets by "/";
//                                                      seed j of the call has the weight j + 1.  per: slots of a batch, 0: all
//   seeds_plan_check chunk
//   seeds_plan_check grid
//
// Exit status 0 and facts ("key=value ... ok"), or 1 and one line that names the first property that does not hold.
#include "fora_seeds_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <utility>

using namespace fora;

[[noreturn]] static void failed(const char *what, const char *cond, int line) {
    std::printf("\nFAILED: %s [%s, line %d]\n", what, cond, line);
    std::exit(1);
}
#define CHECK(cond, what) do { if (!(cond)) failed(what, #cond, __LINE__); } while (0)

static std::vector<std::string> split(const std::string &list, char sep) {
    std::vector<std::string> out;
    if (list == "-") return out;
    for (size_t p = 0;;) {
        const size_t q = list.find(sep, p);
        out.push_back(list.substr(p, q == std::string::npos ? q : q - p));
        if (q == std::string::npos) return out;
        p = q + 1;
    }
}
template <class T> static std::vector<T> numbers(const std::string &list) {
    std::vector<T> out;
    for (const std::string &s : split(list, ',')) out.push_back((T)atoll(s.c_str()));
    return out;
}

static int check_sets(int ns, const char *ptr_arg, const char *seeds_arg) {
    const std::vector<int64_t> set_ptr = numbers<int64_t>(ptr_arg);
    const std::vector<int32_t> seeds = numbers<int32_t>(seeds_arg);
    const char *bad = seed_sets_error(strcmp(ptr_arg, "null") ? set_ptr.data() : nullptr, strcmp(seeds_arg, "null") ? seeds.data() : nullptr, ns);
    std::printf("%s\n", bad ? bad : "fine");
    return 0;
}

static int print_weights(const std::vector<double> *weights, int64_t k) {
    const int64_t set_ptr[2] = {0, k};
    std::vector<uint64_t> wfix;
    const char *bad = seed_weights(set_ptr, weights ? weights->data() : nullptr, 1, wfix);
    if (bad) { std::printf("refused: %s\n", bad); return 0; }
    CHECK(wfix.size() == (size_t)k, "one word per seed");
    for (uint64_t w : wfix) std::printf("%llu\n", (unsigned long long)w);
    return 0;
}

static int check_plan(bool dedup, int per_arg, const char *row_ptr_arg, const char *sets_arg) {
    const std::vector<int64_t> row_ptr = numbers<int64_t>(row_ptr_arg);
    std::vector<int64_t> set_ptr{0};
    std::vector<int32_t> seeds;
    for (const std::string &s : split(sets_arg, '/')) {
        for (int32_t v : numbers<int32_t>(s)) seeds.push_back(v);
        set_ptr.push_back((int64_t)seeds.size());
    }
    const int ns = (int)set_ptr.size() - 1;
    CHECK(!seed_sets_error(set_ptr.data(), seeds.data(), ns), "the sets of the case are fine");
    std::vector<double> weights(seeds.size());
    for (size_t j = 0; j < seeds.size(); j++) weights[j] = (double)(j + 1);
    std::vector<uint64_t> wfix;
    CHECK(!seed_weights(set_ptr.data(), weights.data(), ns, wfix) && wfix.size() == seeds.size(), "weights");
    for (int g = 0; g < ns; g++) // (so a term names its place in the set, not only its seed)
        CHECK(std::set<uint64_t>(wfix.begin() + set_ptr[g], wfix.begin() + set_ptr[g + 1]).size() == (size_t)(set_ptr[g + 1] - set_ptr[g]), "every seed of a set has a word of its own");
    const auto dangling = [&](int32_t s) { return row_ptr[(size_t)s + 1] == row_ptr[(size_t)s]; };

    const SeedSlots p = seed_slots(set_ptr.data(), seeds.data(), wfix.data(), ns, row_ptr.data(), dedup);
    const size_t nl = p.slot_src.size(), nd = p.dang_set.size();
    // per set, the terms in order are the set's (seed, word) pairs: live ones through slot_src, dangling ones by node
    CHECK(p.dang_node.size() == nd && p.dang_w.size() == nd, "the dangling triples are triples");
    size_t iu = 0, id = 0;
    for (int g = 0; g < ns; g++)
        for (int64_t j = set_ptr[g]; j < set_ptr[g + 1]; j++) {
            if (dangling(seeds[j])) {
                CHECK(id < nd && p.dang_set[id] == (uint32_t)g && p.dang_node[id] == seeds[j] && p.dang_w[id] == wfix[(size_t)j], "a dangling seed's term");
                id++;
            } else {
                CHECK(iu < p.uses.size() && p.uses[iu].set == (uint32_t)g && p.uses[iu].slot < nl, "a live seed's use");
                CHECK(p.slot_src[p.uses[iu].slot] == seeds[j] && p.uses[iu].w == wfix[(size_t)j], "a live seed's term: its slot runs the seed");
                iu++;
            }
        }
    CHECK(iu == p.uses.size() && id == nd, "no term beyond the sets'");
    // slots in order of first appearance; one per live id with dedup, one per listed live seed without
    std::vector<int32_t> want_src;
    std::set<int32_t> ids, live_ids;
    for (int32_t s : seeds) {
        ids.insert(s);
        if (!dangling(s) && (!dedup || live_ids.insert(s).second)) want_src.push_back(s);
    }
    CHECK(p.slot_src == want_src, "slots in order of first appearance");
    uint32_t next = 0;
    for (const SeedUse &u : p.uses) { CHECK(u.slot <= next, "a new slot is the next one"); next = std::max(next, u.slot + 1); }
    CHECK(next == nl, "every slot has a use");
    CHECK(p.distinct == ids.size(), "distinct ids");

    // the batches, decoded through the view from vectors of exactly the planned size
    const int per = per_arg > 0 ? per_arg : (int)std::max<size_t>(nl, 1);
    const std::vector<SeedBatch> batches = seed_batches(p.uses, (int)nl, per);
    CHECK(batches.size() == (nl + (size_t)per - 1) / (size_t)per, "batches");
    std::multiset<std::pair<std::pair<uint32_t, uint32_t>, uint64_t>> got, want; // ((set, slot of the call), w)
    for (const SeedUse &u : p.uses) want.insert({{u.set, u.slot}, u.w});
    std::printf("nl=%zu nd=%zu distinct=%llu UT=", nl, nd, (unsigned long long)p.distinct);
    for (size_t bi = 0; bi < batches.size(); bi++) {
        const SeedBatch &b = batches[bi];
        CHECK(b.pack.size() == SeedListView<uint64_t>::words(b.U, b.T), "words of the list");
        CHECK(b.pack.size() * 2 >= 2 * (size_t)b.U + b.U + 2 * (size_t)b.T + 1 && b.pack.size() * 2 <= 2 * (size_t)b.U + b.U + 2 * (size_t)b.T + 2, "U words, then U + 2 T + 1 halves, rounded up");
        const std::vector<uint64_t> copy(b.pack); // (exactly the words: one too far is out of bounds)
        const SeedListView<const uint64_t> l = b.list(copy.data());
        std::vector<uint32_t> halves((size_t)b.U + 2 * (size_t)b.T + 1);
        memcpy(halves.data(), l.use_slot(), halves.size() * 4);
        const uint32_t *slot = halves.data(), *seg = slot + b.U, *set_id = seg + b.T + 1;
        CHECK((const void *)l.seg() == (const void *)(l.use_slot() + b.U) && (const void *)l.set_id() == (const void *)(l.seg() + b.T + 1), "the tables follow each other");
        CHECK(b.U >= 1 && b.T >= 1 && seg[0] == 0 && seg[b.T] == b.U, "seg starts at 0 and ends at U");
        for (uint32_t t = 0; t < b.T; t++) {
            CHECK(seg[t] < seg[t + 1], "seg ascends: no set without a use");
            CHECK(t == 0 || set_id[t - 1] < set_id[t], "the set ids strictly ascend");
            CHECK(set_id[t] < (uint32_t)ns, "a set of the call");
            for (uint32_t i = seg[t]; i < seg[t + 1]; i++) {
                CHECK(slot[i] < (uint32_t)per && bi * (size_t)per + slot[i] < nl, "a slot of the batch");
                got.insert({{set_id[t], (uint32_t)(bi * (size_t)per + slot[i])}, l.use_w()[i]});
            }
        }
        std::printf("%s%u.%u", bi ? "," : "", b.U, b.T);
    }
    CHECK(got == want, "the uses of all batches together are the call's, slot % per inside a batch");
    // the dangling triples
    const std::vector<uint64_t> dpack = seed_dangling_pack(p);
    CHECK(dpack.size() == SeedDanglingView<uint64_t>::words(nd) && dpack.size() == 2 * nd, "words of the dangling triples");
    const SeedDanglingView<const uint64_t> d{dpack.data(), nd};
    if (nd) {
        CHECK(!memcmp(d.w(), p.dang_w.data(), nd * 8) && !memcmp(d.set(), p.dang_set.data(), nd * 4) && !memcmp(d.node(), p.dang_node.data(), nd * 4), "the triples read back");
        CHECK((const void *)d.set() == (const void *)(dpack.data() + nd) && (const void *)d.node() == (const void *)(d.set() + nd), "w, then set, then node");
        CHECK((const char *)(dpack.data() + dpack.size()) - (const char *)(d.node() + nd) == 0, "node ends the words");
    }
    std::printf(" slot_src=");
    for (size_t i = 0; i < nl; i++) std::printf("%s%d", i ? "," : "", p.slot_src[i]);
    std::printf("%s ok\n", nl ? "" : "-");
    return 0;
}

static int check_chunk() {
    int cases = 0;
    for (int64_t opt : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)255, (int64_t)256, (int64_t)65534, (int64_t)65535, (int64_t)1000000})
        for (uint64_t n : {(uint64_t)1, (uint64_t)2, (uint64_t)1001, (uint64_t)1002, (uint64_t)0x7FFFFFFF, (uint64_t)0x7FFFFFFE}) {
            const int C = seeds_chunk(opt, n);
            CHECK(C >= 1 && C <= 65534, "a chunk of 1 .. 65534 rows");
            CHECK(!(n & 1) || ((uint64_t)C * n) % 2 == 0, "odd n: every chunk starts at an even word");
            const int64_t asked = std::min<int64_t>(std::max<int64_t>(opt, 1), 65534);
            CHECK(C == asked || (C == asked + 1 && (n & 1) && (asked & 1)), "the option's value, or one more to make it even");
            cases++;
        }
    std::printf("cases=%d ok\n", cases);
    return 0;
}

static int check_grid() {
    const uint64_t tile = (uint64_t)SC_TILE;
    int cases = 0;
    for (uint64_t n : {(uint64_t)1, tile, 2 * tile + 1, 1024 * 2 * tile, 1024 * 2 * tile + 1, (uint64_t)0x7FFFFFFF}) {
        const CompactGeom g = seed_combine_geom(n);
        const uint64_t R = g.R, X = g.X;
        CHECK(R % tile == 0 && R >= 2 * tile, "R: whole tiles, at least two");
        CHECK(X >= 1 && (X - 1) * R < n && n <= X * R, "X workgroups of R ids cover n, and none is idle");
        CHECK(X <= 1024, "at most 1024 workgroups per set");
        // the expressions of seed_combine before there was a function
        const uint32_t R0 = (uint32_t)std::max<uint64_t>(2 * tile, ((n + 1023) / 1024 + tile - 1) / tile * tile);
        CHECK(g.R == R0 && g.X == (uint32_t)((n + R0 - 1) / R0), "the grid seed_combine spelt out");
        cases++;
    }
    std::printf("cases=%d tile=%llu ok\n", cases, (unsigned long long)tile);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "sets")) return check_sets(atoi(argv[2]), argv[3], argv[4]);
    if (argc == 3 && !strcmp(argv[1], "uniform")) return print_weights(nullptr, atoll(argv[2]));
    if (argc >= 3 && !strcmp(argv[1], "weights")) {
        std::vector<double> w;
        for (int i = 2; i < argc; i++) w.push_back(strtod(argv[i], nullptr)); // (hex floats, "nan" and "inf" too)
        return print_weights(&w, (int64_t)w.size());
    }
    if (argc == 6 && !strcmp(argv[1], "plan")) return check_plan(atoi(argv[2]) != 0, atoi(argv[3]), argv[4], argv[5]);
    if (argc == 2 && !strcmp(argv[1], "chunk")) return check_chunk();
    if (argc == 2 && !strcmp(argv[1], "grid")) return check_grid();
    std::printf("usage: seeds_plan_check sets <ns> <set_ptr> <seeds> | uniform <k> | weights <value> ... | plan <dedup> <per> <row_ptr> <sets> | chunk | grid\n");
    return 2;
}
