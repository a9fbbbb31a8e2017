// attn_plan_check.cpp -- the host side of ATTENTION (fora_amd/csrc/fora_attn_plan.h) against brute force, without a GPU.
// Built with -fsanitize=address,undefined by tests/test_attention_cpu.py and run directly.
//
//   attn_plan_check <attn_short> <prop_segs> <len,len,...|->   the short list and the longer rows' plan of rows of these lengths
#include "fora_attn_plan.h"

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
    if (argc != 4) { fprintf(stderr, "usage: attn_plan_check <attn_short> <prop_segs> <lens>\n"); return 2; }
    const int64_t option = atoll(argv[1]);
    const uint64_t per = (uint64_t)std::max<int64_t>(atoll(argv[2]), 1);
    const std::vector<int64_t> lens = parse_list(argv[3]);
    const int nq = (int)lens.size();
    std::vector<int64_t> row_ptr((size_t)nq + 1, 0);
    for (int i = 0; i < nq; i++) row_ptr[(size_t)i + 1] = row_ptr[(size_t)i] + lens[(size_t)i];
    const uint32_t cap = attn_short_cap(option);
    CHECK(cap <= 256 && (option < 0 ? cap == 0 : option > 256 ? cap == 256 : cap == (uint32_t)option));
    const AttnPlan p = attn_plan(row_ptr.data(), nq, cap, per);
    // ---- brute force: the counts
    uint64_t short_rows = 0, long_rows = 0, empty = 0, max_row = 0, segments = 0, long_segs = 0;
    for (int i = 0; i < nq; i++) {
        const uint64_t L = (uint64_t)lens[(size_t)i];
        max_row = std::max(max_row, L);
        segments += (L + 255) / 256;
        if (!L) empty++;
        else if (L <= cap) short_rows++;
        if (L > cap) { long_rows++; long_segs += (L + 255) / 256; }
    }
    CHECK(p.short_rows == short_rows && p.long_rows == long_rows && p.max_row == max_row && p.segments == segments);
    CHECK(p.entries == (uint64_t)row_ptr[(size_t)nq]);
    CHECK(p.shrt.size() == short_rows + empty && p.lrows.size() == long_rows && p.lng.segs.size() == long_segs);
    // ---- every row is in exactly one of the two row lists, in row order, as it is
    std::vector<int> seen((size_t)nq, 0);
    std::vector<int> covered((size_t)row_ptr[(size_t)nq], 0);
    int last = -1;
    for (const PropSeg &s : p.shrt) {
        CHECK(s.row > last && s.row < nq);
        last = s.row;
        CHECK(s.first == row_ptr[(size_t)s.row] && (int64_t)s.len == lens[(size_t)s.row] && s.len <= cap);
        seen[(size_t)s.row]++;
        for (uint32_t k = 0; k < s.len; k++) covered[(size_t)(s.first + k)]++;
    }
    last = -1;
    for (const PropSeg &s : p.lrows) {
        CHECK(s.row > last && s.row < nq);
        last = s.row;
        CHECK(s.first == row_ptr[(size_t)s.row] && (int64_t)s.len == lens[(size_t)s.row] && s.len > cap);
        seen[(size_t)s.row]++;
    }
    for (int c : seen) CHECK(c == 1);
    // ---- the longer rows' plan: segments in row order, consecutive cuts of 256; chunks of at most `per`; records that name
    // exactly the slots of their row's segments in the chunk, first and last flagged
    CHECK(long_rows ? p.lng.chunks.size() == std::max<uint64_t>(1, (long_segs + per - 1) / per) : p.lng.chunks.size() == 1 || nq == 0);
    CHECK(p.lng.entries + [&] { uint64_t e = 0; for (const PropSeg &s : p.shrt) e += s.len; return e; }() == p.entries);
    uint64_t seg_at = 0, rec_at = 0;
    std::vector<uint64_t> done((size_t)nq, 0); // segments of a row seen so far
    for (size_t ci = 0; ci < p.lng.chunks.size(); ci++) {
        const PropChunk &ch = p.lng.chunks[ci];
        CHECK(ch.seg0 == seg_at && ch.rec0 == rec_at && ch.nseg <= per);
        if (ci + 1 < p.lng.chunks.size()) CHECK(ch.nseg == per);
        uint64_t slot = 0;
        for (uint64_t r = 0; r < ch.nrec; r++) {
            const PropRowRec &rec = p.lng.recs[(size_t)(ch.rec0 + r)];
            CHECK(rec.row >= 0 && rec.row < nq && (uint64_t)lens[(size_t)rec.row] > cap && rec.nseg >= 1);
            const uint64_t ns = ((uint64_t)lens[(size_t)rec.row] + 255) / 256;
            CHECK(rec.slot0 == slot && slot + rec.nseg <= ch.nseg);
            CHECK(((rec.flags & PROP_FIRST) != 0) == (done[(size_t)rec.row] == 0));
            CHECK(((rec.flags & PROP_LAST) != 0) == (done[(size_t)rec.row] + rec.nseg == ns));
            for (uint32_t k = 0; k < rec.nseg; k++) {
                const PropSeg &s = p.lng.segs[(size_t)(ch.seg0 + slot + k)];
                const uint64_t at = (done[(size_t)rec.row] + k) * 256;
                CHECK(s.row == rec.row && s.slot == slot + k && s.first == row_ptr[(size_t)rec.row] + (int64_t)at);
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
    for (int i = 0; i < nq; i++) CHECK(done[(size_t)i] == ((uint64_t)lens[(size_t)i] > cap ? ((uint64_t)lens[(size_t)i] + 255) / 256 : 0));
    for (int c : covered) CHECK(c == 1);
    // ---- the vector width of the product: what every head's slice allows
    static const uint32_t wf[] = {4, 2, 1}, wb[] = {8, 4, 1};
    for (int heads = 1; heads <= 3; heads++)
        for (int dv = 1; dv <= 40; dv++)
            for (uint64_t addr = 0; addr < 32; addr += 2)
                for (int64_t ld = (int64_t)heads * dv; ld < (int64_t)heads * dv + 9; ld++)
                    for (int b = 0; b < 2; b++) {
                        const uint32_t elt = b ? 2 : 4;
                        if (addr % elt) continue;
                        const uint32_t V = attn_vec_width(addr, ld, dv, heads, elt, b ? wb : wf, 3);
                        uint32_t want = 1;
                        for (int i = 0; i < 3; i++) {
                            const uint32_t W = (b ? wb : wf)[i];
                            bool ok = W == 1 || (W <= (uint32_t)dv && ld % W == 0);
                            for (int h = 0; ok && W > 1 && h < heads; h++) ok = (addr + (uint64_t)h * dv * elt) % ((uint64_t)W * elt) == 0;
                            if (ok) { want = W; break; }
                        }
                        CHECK(V == want);
                    }
    printf("short=%llu long_segs=%llu short_rows=%llu long_rows=%llu chunks=%llu ok\n", (unsigned long long)p.shrt.size(), (unsigned long long)long_segs,
           (unsigned long long)p.short_rows, (unsigned long long)p.long_rows, (unsigned long long)p.lng.chunks.size());
    return 0;
}
