// attn_bwd_plan_check.cpp -- the column side of ATTENTION, BACKWARD (fora_amd/csrc/fora_attn_bwd_plan.h) against brute force,
// without a GPU.  Built with -fsanitize=address,undefined by tests/test_attention_bwd_cpu.py and run directly.
//
//   attn_bwd_plan_check <attn_short> <chunk_segs> <len,len,...|->   the short list and the longer columns' plan of columns of
//                                                                   these lengths
#include "fora_attn_bwd_plan.h"

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
    if (argc != 4) { fprintf(stderr, "usage: attn_bwd_plan_check <attn_short> <chunk_segs> <lens>\n"); return 2; }
    const int64_t option = atoll(argv[1]);
    const uint64_t per = (uint64_t)std::max<int64_t>(atoll(argv[2]), 1);
    const std::vector<int64_t> lens = parse_list(argv[3]);
    const int64_t n = (int64_t)lens.size();
    std::vector<int64_t> col_ptr((size_t)n + 1, 0);
    for (int64_t v = 0; v < n; v++) col_ptr[(size_t)v + 1] = col_ptr[(size_t)v] + lens[(size_t)v];
    const uint32_t cap = attn_short_cap(option);
    const AttnColPlan p = attn_col_plan(col_ptr.data(), n, cap, per);
    // ---- brute force: the counts
    uint64_t columns = 0, short_cols = 0, long_cols = 0, max_col = 0, long_segs = 0, long_entries = 0;
    for (int64_t v = 0; v < n; v++) {
        const uint64_t L = (uint64_t)lens[(size_t)v];
        max_col = std::max(max_col, L);
        if (L) columns++;
        if (L && L <= cap) short_cols++;
        if (L > cap) { long_cols++; long_segs += (L + 255) / 256; long_entries += L; }
    }
    CHECK(p.columns == columns && p.short_cols == short_cols && p.long_cols == long_cols && p.max_col == max_col);
    CHECK(p.shrt.size() == short_cols && p.lng.segs.size() == long_segs && p.lng.entries == long_entries);
    CHECK(attn_long_col_segs(col_ptr.data(), n, cap) == long_segs);
    // ---- the short list: every non-empty column of at most cap entries once, in column order, as it is; no empty column
    std::vector<int> seen((size_t)n, 0);
    std::vector<int> covered((size_t)col_ptr[(size_t)n], 0);
    int64_t last = -1;
    for (const PropSeg &s : p.shrt) {
        CHECK(s.row > last && s.row < n);
        last = s.row;
        CHECK(s.first == col_ptr[(size_t)s.row] && (int64_t)s.len == lens[(size_t)s.row] && s.len >= 1 && s.len <= cap && s.len <= 256);
        seen[(size_t)s.row]++;
        for (uint32_t k = 0; k < s.len; k++) covered[(size_t)(s.first + k)]++;
    }
    // ---- the longer columns' plan: segments in column order, consecutive cuts of 256; chunks of at most `per`; records that
    // name exactly the slots of their column's segments in the chunk, first and last flagged; no record for any other column
    CHECK(n == 0 ? p.lng.chunks.empty() : p.lng.chunks.size() == std::max<uint64_t>(1, (long_segs + per - 1) / per));
    uint64_t seg_at = 0, rec_at = 0;
    std::vector<uint64_t> done((size_t)n, 0); // segments of a column seen so far
    for (size_t ci = 0; ci < p.lng.chunks.size(); ci++) {
        const PropChunk &ch = p.lng.chunks[ci];
        CHECK(ch.seg0 == seg_at && ch.rec0 == rec_at && ch.nseg <= per);
        if (ci + 1 < p.lng.chunks.size()) CHECK(ch.nseg == per);
        uint64_t slot = 0;
        for (uint64_t r = 0; r < ch.nrec; r++) {
            const PropRowRec &rec = p.lng.recs[(size_t)(ch.rec0 + r)];
            CHECK(rec.row >= 0 && rec.row < n && (uint64_t)lens[(size_t)rec.row] > cap && rec.nseg >= 1);
            const uint64_t ns = ((uint64_t)lens[(size_t)rec.row] + 255) / 256;
            CHECK(rec.slot0 == slot && slot + rec.nseg <= ch.nseg);
            CHECK(((rec.flags & PROP_FIRST) != 0) == (done[(size_t)rec.row] == 0));
            CHECK(((rec.flags & PROP_LAST) != 0) == (done[(size_t)rec.row] + rec.nseg == ns));
            if (rec.flags & PROP_FIRST) seen[(size_t)rec.row]++;
            for (uint32_t k = 0; k < rec.nseg; k++) {
                const PropSeg &s = p.lng.segs[(size_t)(ch.seg0 + slot + k)];
                const uint64_t at = (done[(size_t)rec.row] + k) * 256;
                CHECK(s.row == rec.row && s.slot == slot + k && s.first == col_ptr[(size_t)rec.row] + (int64_t)at);
                CHECK(s.len == std::min<uint64_t>(256, (uint64_t)lens[(size_t)rec.row] - at));
                for (uint32_t j = 0; j < s.len; j++) covered[(size_t)(s.first + j)]++;
            }
            done[(size_t)rec.row] += rec.nseg;
            slot += rec.nseg;
        }
        CHECK(slot == ch.nseg);
        seg_at += ch.nseg;
        rec_at += ch.nrec;
    }
    CHECK(seg_at == long_segs && rec_at == p.lng.recs.size());
    for (int64_t v = 0; v < n; v++) {
        CHECK(done[(size_t)v] == ((uint64_t)lens[(size_t)v] > cap ? ((uint64_t)lens[(size_t)v] + 255) / 256 : 0));
        CHECK(seen[(size_t)v] == (lens[(size_t)v] ? 1 : 0)); // a non-empty column is in exactly one list, an empty one in none
    }
    for (int c : covered) CHECK(c == 1);
    // ---- the lane groups of k_attn_cols: the smallest power of two of lanes that holds the slice, tiles that cover it
    for (uint32_t V : {1u, 2u, 4u, 8u})
        for (int w = (int)V; w <= 1100; w += (w < 140 ? 1 : 97)) {
            const PropGeom g = attn_cols_geom(V, w);
            const uint32_t lanes = ((uint32_t)w + V - 1) / V;
            CHECK(g.V == V && g.G >= 1 && g.G <= 64 && (g.G & (g.G - 1)) == 0 && g.segs_per_wave * g.G == 64);
            CHECK(g.G >= std::min(lanes, 64u) && (g.G == 1 || g.G / 2 < lanes));
            CHECK((uint64_t)g.tiles * g.G * V >= (uint32_t)w && (uint64_t)(g.tiles - 1) * g.G * V < (uint32_t)w);
        }
    printf("short=%llu long_cols=%llu long_segs=%llu columns=%llu chunks=%llu ok\n", (unsigned long long)p.shrt.size(), (unsigned long long)long_cols,
           (unsigned long long)long_segs, (unsigned long long)columns, (unsigned long long)p.lng.chunks.size());
    return 0;
}
