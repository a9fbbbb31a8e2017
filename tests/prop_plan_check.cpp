// prop_plan_check.cpp -- the host side of PROPAGATE (fora_amd/csrc/fora_prop_plan.h) against brute force, without a GPU.
// Built with -fsanitize=address,undefined by tests/test_propagate_cpu.py and run directly.
//
//   prop_plan_check plan <option> <free_bytes> <d> <len,len,...|->   the plan of rows of these lengths; prints its facts
//   prop_plan_check rowptr                                           prop_row_ptr_ok on good and bad arrays
//   prop_plan_check geom                                             prop_geom: alignment, widths, lane groups
//   prop_plan_check helpers                                          widths, group exponent, byte extents, long-row segments
#include "fora_prop_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

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

static int check_plan(int64_t option, uint64_t free_bytes, int d, const std::vector<int64_t> &lens) {
    const int nq = (int)lens.size();
    std::vector<int64_t> row_ptr((size_t)nq + 1, 0);
    for (int i = 0; i < nq; i++) row_ptr[(size_t)i + 1] = row_ptr[(size_t)i] + lens[(size_t)i];
    CHECK(prop_row_ptr_ok(row_ptr.data(), nq, (uint64_t)row_ptr[(size_t)nq]));
    // brute force: the segments of every row, entry by entry
    struct Seg { int row; int64_t first; uint32_t len; };
    std::vector<Seg> want;
    uint64_t max_row = 0;
    for (int i = 0; i < nq; i++) {
        max_row = std::max<uint64_t>(max_row, (uint64_t)lens[(size_t)i]);
        for (int64_t e = row_ptr[(size_t)i]; e < row_ptr[(size_t)i + 1]; e++) {
            if ((e - row_ptr[(size_t)i]) % 256 == 0) want.push_back(Seg{i, e, 0});
            want.back().len++;
        }
    }
    CHECK(prop_segments(row_ptr.data(), nq) == want.size());
    const uint64_t per = prop_chunk_segs(option, want.size(), free_bytes, d);
    CHECK(per >= 1 && per <= std::max<uint64_t>(want.size(), 1));
    if (option > 0) CHECK(per == std::min<uint64_t>((uint64_t)option, std::max<uint64_t>(want.size(), 1)));
    else CHECK(per == std::min<uint64_t>(std::max<uint64_t>(1, free_bytes / 4 / ((uint64_t)d * 8 + 8)), std::max<uint64_t>(want.size(), 1)));
    const PropPlan p = prop_plan(row_ptr.data(), nq, per);
    CHECK(p.entries == (uint64_t)row_ptr[(size_t)nq] && p.max_row == max_row);
    CHECK(p.segs.size() == want.size());
    CHECK(p.chunks.size() == (nq ? std::max<uint64_t>(1, (want.size() + per - 1) / per) : 0));
    // the segments: row order, the brute-force cuts, the slot = the position inside the chunk
    uint64_t seg = 0, rec = 0;
    std::vector<uint64_t> done((size_t)nq, 0), total((size_t)nq, 0);
    std::vector<int> finished((size_t)nq, 0);
    for (int i = 0; i < nq; i++) total[(size_t)i] = ((uint64_t)lens[(size_t)i] + 255) / 256;
    int next_row = 0; // rows are finished in ascending order, each once
    for (size_t ci = 0; ci < p.chunks.size(); ci++) {
        const PropChunk &ch = p.chunks[ci];
        CHECK(ch.seg0 == seg && ch.rec0 == rec && ch.nseg <= per);
        if (ci + 1 < p.chunks.size()) CHECK(ch.nseg == per); // only the last chunk is short
        for (uint64_t k = 0; k < ch.nseg; k++) {
            const PropSeg &s = p.segs[(size_t)(seg + k)];
            const Seg &w = want[(size_t)(seg + k)];
            CHECK(s.row == w.row && s.first == w.first && s.len == w.len && s.slot == k && s.len >= 1 && s.len <= PROP_SEG);
        }
        // the records: they walk the chunk's slots in order without a gap; a row continues only across a chunk's edge
        uint64_t slot = 0;
        for (uint64_t k = 0; k < ch.nrec; k++) {
            CHECK(rec + k < p.recs.size());
            const PropRowRec &r = p.recs[(size_t)(rec + k)];
            CHECK(r.row >= 0 && r.row < nq && r.row == next_row);
            CHECK(((r.flags & PROP_FIRST) != 0) == (done[(size_t)r.row] == 0));
            if (!(r.flags & PROP_FIRST)) CHECK(k == 0 && ci > 0);
            if (!(r.flags & PROP_LAST)) CHECK(k + 1 == ch.nrec && ci + 1 < p.chunks.size());
            if (r.nseg) CHECK(r.slot0 == slot);
            for (uint32_t j = 0; j < r.nseg; j++) CHECK(p.segs[(size_t)(seg + slot + j)].row == r.row);
            slot += r.nseg;
            done[(size_t)r.row] += r.nseg;
            CHECK(((r.flags & PROP_LAST) != 0) == (done[(size_t)r.row] == total[(size_t)r.row]));
            if (r.flags & PROP_LAST) { finished[(size_t)r.row]++; next_row++; }
            if (!total[(size_t)r.row]) CHECK(r.nseg == 0 && r.flags == (PROP_FIRST | PROP_LAST));
            else CHECK(r.nseg >= 1);
        }
        CHECK(slot == ch.nseg);
        seg += ch.nseg; rec += ch.nrec;
    }
    CHECK(seg == p.segs.size() && rec == p.recs.size() && next_row == nq);
    for (int i = 0; i < nq; i++) CHECK(finished[(size_t)i] == 1);
    printf("segments=%zu per=%llu chunks=%zu recs=%zu max_row=%llu entries=%llu ok\n", p.segs.size(), (unsigned long long)per, p.chunks.size(), p.recs.size(),
           (unsigned long long)p.max_row, (unsigned long long)p.entries);
    return 0;
}

static int check_rowptr() {
    const int64_t good[] = {0, 3, 3, 10}, dec[] = {0, 5, 4, 10}, first[] = {1, 3, 3, 10}, zero[] = {0};
    CHECK(prop_row_ptr_ok(good, 3, 10));
    CHECK(!prop_row_ptr_ok(good, 3, 9) && !prop_row_ptr_ok(good, 3, 11)); // off by one at the end
    CHECK(!prop_row_ptr_ok(dec, 3, 10) && !prop_row_ptr_ok(first, 3, 10));
    CHECK(!prop_row_ptr_ok(nullptr, 3, 10) && !prop_row_ptr_ok(good, -1, 10));
    CHECK(prop_row_ptr_ok(zero, 0, 0) && !prop_row_ptr_ok(zero, 0, 1));
    CHECK(prop_row_ptr_ok(good, 2, 3));
    printf("ok\n");
    return 0;
}

static int check_geom() {
    const uint32_t *const f32 = prop_widths(false), *const bf16 = prop_widths(true);
    int cases = 0;
    for (int d : {1, 2, 3, 4, 16, 63, 64, 65, 128, 130, 256, 257, 4096, 65536})
        for (uint64_t addr : {0ull, 2ull, 4ull, 8ull, 16ull})
            for (int64_t pad : {0, 1, 2, 3, 4, 8})
                for (int t = 0; t < 2; t++) {
                    const uint32_t elt = t ? 2 : 4;
                    if (addr % elt) continue;
                    const int64_t ldf = d + pad;
                    const PropGeom g = prop_geom(addr, ldf, d, elt, t ? bf16 : f32, 3);
                    CHECK(g.V == 1 || (addr % (g.V * elt) == 0 && ldf % g.V == 0 && g.V <= (uint32_t)d)); // a vector load is aligned in every row
                    CHECK(g.G >= 1 && g.G <= 64 && (g.G & (g.G - 1)) == 0 && g.segs_per_wave * g.G == 64);
                    CHECK((uint64_t)g.tiles * g.G * g.V >= (uint64_t)d);                          // every column has a lane
                    CHECK((uint64_t)(g.tiles - 1) * g.G * g.V < (uint64_t)d);                    // no tile without a column
                    if (g.tiles == 1 && g.G > 1) CHECK((uint64_t)(g.G / 2) * g.V < (uint64_t)d); // the smallest group that holds a row
                    if (d <= 3) CHECK(g.segs_per_wave >= 16);                                     // narrow rows do not idle a wave
                    // the widest legal width is the one taken
                    for (int i = 0; i < 3; i++) {
                        const uint32_t V = (t ? bf16 : f32)[i];
                        if (V > g.V) CHECK(!(V <= (uint32_t)d && addr % (V * elt) == 0 && ldf % V == 0));
                    }
                    cases++;
                }
    printf("cases=%d ok\n", cases);
    return 0;
}

// the pure helpers of the drivers, each against a restatement that shares no code with it
static int check_helpers() {
    // the widths: three per element type, descending, ending in 1, 16 bytes a lane at most
    CHECK(PROP_NWIDTHS == 3);
    for (int t = 0; t < 2; t++) {
        const uint32_t *w = prop_widths(t != 0), elt = t ? 2 : 4;
        CHECK(w[0] * elt == 16 && w[0] > w[1] && w[1] > w[2] && w[2] == 1);
    }
    CHECK(prop_widths(false)[1] == 2 && prop_widths(true)[1] == 4);
    // the group exponent: the smallest lg <= 6 with 2^lg >= d, by trying every lg
    for (uint32_t d : {1u, 2u, 3u, 4u, 5u, 31u, 32u, 33u, 63u, 64u, 65u, 4096u, 65536u}) {
        uint32_t want = 6;
        for (uint32_t lg = 0; lg <= 6; lg++)
            if ((1ull << lg) >= d) { want = lg; break; }
        CHECK(prop_group_lg(d) == want);
    }
    CHECK(prop_group_lg(1) == 0 && prop_group_lg(2) == 1 && prop_group_lg(63) == 6 && prop_group_lg(64) == 6 && prop_group_lg(65) == 6 && prop_group_lg(65536) == 6);
    // the byte extents: one past the offset of the last element that is read, by walking the elements
    for (uint64_t rows : {0ull, 1ull, 2ull, 7ull})
        for (uint64_t width : {1ull, 3ull, 8ull})
            for (uint64_t pad : {0ull, 1ull, 5ull})
                for (uint32_t elt : {2u, 4u, 8u}) {
                    const uint64_t ld = width + pad;
                    uint64_t end = 0;
                    for (uint64_t r = 0; r < rows; r++)
                        for (uint64_t col = 0; col < width; col++) end = std::max(end, (r * ld + col + 1) * elt);
                    CHECK(prop_matrix_bytes(rows, ld, width, elt) == end);
                    CHECK(prop_vector_bytes(rows * width, elt) == rows * width * elt);
                }
    CHECK(prop_matrix_bytes(0, 1000, 10, 4) == 0 && prop_matrix_bytes(1, 1000, 10, 4) == 40 && prop_matrix_bytes(2, 1000, 10, 4) == 4040);
    CHECK(prop_matrix_bytes(2, 10, 10, 2) == 40 && prop_vector_bytes(0, 8) == 0);
    // the long-row segments: entry by entry, for caps at, one below and one above the rows' lengths
    const std::vector<int64_t> lens = {0, 1, 5, PROP_SEG - 1, PROP_SEG, PROP_SEG + 1, 2 * PROP_SEG, 2 * PROP_SEG + 1, 600, 0, 3};
    std::vector<int64_t> row_ptr(lens.size() + 1, 0);
    for (size_t i = 0; i < lens.size(); i++) row_ptr[i + 1] = row_ptr[i] + lens[i];
    const int nq = (int)lens.size();
    std::vector<uint32_t> caps = {0, 0xFFFFFFFFu};
    for (int64_t L : lens)
        for (int64_t c = L - 1; c <= L + 1; c++)
            if (c >= 0) caps.push_back((uint32_t)c);
    for (uint32_t cap : caps) {
        uint64_t want = 0;
        for (int i = 0; i < nq; i++) {
            if ((uint64_t)lens[(size_t)i] <= cap) continue;
            for (int64_t e = 0; e < lens[(size_t)i]; e++) want += e % PROP_SEG == 0;
        }
        CHECK(prop_long_segments(row_ptr.data(), nq, cap) == want);
    }
    CHECK(prop_long_segments(row_ptr.data(), nq, 0) == prop_segments(row_ptr.data(), nq) && prop_long_segments(row_ptr.data(), 0, 0) == 0);
    printf("caps=%zu ok\n", caps.size());
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 6 && !strcmp(argv[1], "plan")) return check_plan(atoll(argv[2]), strtoull(argv[3], nullptr, 10), atoi(argv[4]), parse_list(argv[5]));
    if (argc >= 2 && !strcmp(argv[1], "rowptr")) return check_rowptr();
    if (argc >= 2 && !strcmp(argv[1], "geom")) return check_geom();
    if (argc >= 2 && !strcmp(argv[1], "helpers")) return check_helpers();
    fprintf(stderr, "usage: prop_plan_check plan <option> <free_bytes> <d> <lens> | rowptr | geom | helpers\n");
    return 2;
}
