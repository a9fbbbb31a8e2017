// flush_plan_check.cpp -- the line-aligned flush of k_walk_dg's result stages (fora_flush_plan.h) restated on the CPU the way
// stage_flush<.., ONE, G> uses it: the waves of a workgroup share one fill counter per bin, each wave appends up to 64 results
// at a time to its stage and flushes when fewer than 64 slots are free; a flush counts and ranks its results per bin, sends
// flush_send() of each bin to the sub-bucket (one returning add on the fill), rebuilds the stage through FlushBin::slot and
// keeps the rest; a flush that would keep more than the cap sends everything, and so does the closing flush of every wave.
// For random bin populations, starting fills, caps, G = 8 and 16, 1 to 128 bins, waves flushing in any order:
//   every result leaves exactly once, to the sub-bucket of its bin;
//   positions inside a sub-bucket are distinct, start at the starting fill and end below the final count (no holes);
//   a run of a flush that is neither full nor closing ends on a multiple of G, and starts on one unless it is the run that
//   brings an unaligned fill (the starting fill, or what a full or closing flush left) back to a line boundary;
//   the rebuilt stage is a permutation of its slots, the kept results stay sorted by bin, at most G - 1 a bin;
//   the stage never holds more than ST - 64 results after a flush.
// Built with -fsanitize=address,undefined by tests/test_flush_plan_cpu.py.
#include "fora_flush_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fora;

static_assert(flush_head(0, 8) == 0 && flush_head(5, 8) == 3 && flush_head(16, 16) == 0 && flush_head(17, 16) == 15, "head");
static_assert(flush_send(2, 5, 8) == 0 && flush_send(3, 5, 8) == 3 && flush_send(12, 5, 8) == 11 && flush_send(9, 0, 8) == 8 && flush_send(7, 8, 8) == 0, "send");
static_assert(flush_keep_cap(384, 0) == 192 && flush_keep_cap(384, 16) == 16 && flush_keep_cap(384, 384) == 320 && flush_keep_cap(128, 0) == 64, "cap");
static_assert(FlushBin::make(11, 7, 300).sent() == 11 && FlushBin::make(11, 7, 300).kept_before() == 7 && FlushBin::make(11, 7, 300).sent_before() == 300, "bin word");
static_assert(FlushBin::make(8, 5, 40).slot(3, 20) == 63 && FlushBin::make(8, 5, 40).slot(9, 20) == 6, "sent behind the kept ones; kept by bin from slot 0");

#define CHECK(c) do { if (!(c)) { printf("line %d: %s (G=%u nbins=%u ST=%u keep=%u seed=%u)\n", __LINE__, #c, G, nbins, ST, keep_opt, seed); return 1; } } while (0)

struct Rng {
    uint32_t s;
    uint32_t next() { s = s * 1664525u + 1013904223u; return s >> 8; }
};

struct Wave {
    std::vector<uint64_t> stage; // result = id << 8 | bin
    uint32_t count = 0;
};

static int run(uint32_t G, uint32_t nbins, uint32_t ST, uint32_t keep_opt, uint32_t nw, uint32_t per_wave, int skew, uint32_t seed, uint64_t &flushes, uint64_t &fulls) {
    Rng rng{seed};
    const uint32_t cap = flush_keep_cap(ST, keep_opt);
    CHECK(cap <= ST - FLUSH_ROOM);
    std::vector<uint32_t> fill(nbins), fill0(nbins);
    for (uint32_t b = 0; b < nbins; b++) fill0[b] = fill[b] = (seed & 1) ? rng.next() % 1000 : 0; // (what the indexed walks left, or nothing)
    std::vector<std::vector<uint64_t>> bucket(nbins);   // the sub-bucket behind its starting fill; 0: not written
    std::vector<Wave> waves(nw);
    for (auto &w : waves) w.stage.assign(ST, 0);
    std::vector<uint32_t> left(nw, per_wave);
    uint64_t next_id = 1, sent_total = 0;

    auto flush = [&](Wave &w, bool all) -> int {
        std::vector<uint32_t> c(nbins, 0), rank(w.count);
        for (uint32_t m = 0; m < w.count; m++) rank[m] = c[w.stage[m] & 0xFF]++;
        std::vector<uint32_t> s(nbins);
        uint32_t kept = 0;
        for (uint32_t b = 0; b < nbins; b++) { s[b] = all ? c[b] : flush_send(c[b], fill[b], G); CHECK(s[b] <= c[b]); CHECK(all || c[b] - s[b] < G); kept += c[b] - s[b]; }
        const bool full = !all && flush_full(kept, cap);
        if (full) { s = c; kept = 0; fulls++; }
        std::vector<FlushBin> word(nbins);
        std::vector<uint32_t> base(nbins);
        uint32_t kb = 0, sb = 0;
        for (uint32_t b = 0; b < nbins; b++) {
            word[b] = FlushBin::make(s[b], kb, sb);
            CHECK(word[b].sent() == s[b] && word[b].kept_before() == kb && word[b].sent_before() == sb);
            base[b] = fill[b];
            if (s[b] && !all && !full) { // an aligned run
                CHECK((fill[b] + s[b]) % G == 0);
                CHECK(fill[b] % G == 0 || s[b] >= flush_head(fill[b], G));
                if (fill[b] % G == 0) CHECK(s[b] % G == 0);
            }
            fill[b] += s[b]; // the one returning add
            kb += c[b] - s[b]; sb += s[b];
        }
        CHECK(kb == kept && sb + kept == w.count);
        std::vector<uint64_t> out(ST, 0); // every result is in registers: the stage is rebuilt
        for (uint32_t m = 0; m < w.count; m++) {
            const uint32_t b = (uint32_t)(w.stage[m] & 0xFF), slot = word[b].slot(rank[m], kept);
            CHECK(slot < w.count && out[slot] == 0);
            CHECK(word[b].sends(rank[m]) == (slot >= kept));
            out[slot] = w.stage[m];
        }
        for (uint32_t m = kept; m < w.count; m++) { // the store loop: slot m of bin b goes to (base - first sent slot) + m
            const uint32_t b = (uint32_t)(out[m] & 0xFF);
            const uint32_t pos = base[b] - (kept + word[b].sent_before()) + m;
            CHECK(pos >= fill0[b] && pos < fill[b]);
            auto &bk = bucket[b];
            if (bk.size() <= pos - fill0[b]) bk.resize(pos - fill0[b] + 1, 0);
            CHECK(bk[pos - fill0[b]] == 0);
            bk[pos - fill0[b]] = out[m];
            sent_total++;
        }
        for (uint32_t m = 1; m < kept; m++) CHECK((out[m - 1] & 0xFF) <= (out[m] & 0xFF));
        w.stage = out;
        w.count = kept;
        CHECK(w.count <= ST - FLUSH_ROOM);
        flushes++;
        return 0;
    };

    uint32_t running = nw;
    while (running) {
        uint32_t wi = rng.next() % nw; // which wave moves next: any order
        while (!left[wi] && !waves[wi].count) wi = (wi + 1) % nw; // (running: some wave has walks or results left)
        Wave &w = waves[wi];
        if (!left[wi]) { // out of walks: the closing flush
            if (flush(w, true)) return 1;
            CHECK(w.count == 0);
        } else {
            uint32_t add = rng.next() % 65; // one emit: up to a wave's 64 results
            if (add > left[wi]) add = left[wi];
            left[wi] -= add;
            for (uint32_t k = 0; k < add; k++) {
                uint32_t b = rng.next() % nbins;
                if (skew == 1 && rng.next() % 4) b = b % (nbins < 3 ? nbins : 3);  // most results in a few bins
                if (skew == 2) b = (b * b) % nbins;
                CHECK(w.count < ST);
                w.stage[w.count++] = (next_id++ << 8) | b;
            }
            if (w.count > ST - FLUSH_ROOM && flush(w, false)) return 1;
        }
        running = 0;
        for (uint32_t k = 0; k < nw; k++) running += left[k] || waves[k].count;
    }
    // every result left exactly once: ids are distinct and none is missing, sub-buckets have no holes
    CHECK(sent_total == next_id - 1);
    std::vector<uint8_t> seen(next_id, 0);
    for (uint32_t b = 0; b < nbins; b++) {
        CHECK(bucket[b].size() == fill[b] - fill0[b]);
        for (uint64_t e : bucket[b]) {
            CHECK(e != 0 && (e & 0xFF) == b);
            CHECK(seen[e >> 8] == 0);
            seen[e >> 8] = 1;
        }
    }
    for (uint64_t i = 1; i < next_id; i++) CHECK(seen[i] == 1);
    return 0;
}

int main(int argc, char **argv) {
    const uint32_t rounds = argc > 1 ? (uint32_t)atoi(argv[1]) : 6;
    const uint32_t bins[] = {1, 2, 3, 35, 64, 65, 128};
    const uint32_t stages[] = {384, 320, 128};
    const uint32_t keeps[] = {0, 1, 16, 100, 1000};
    uint64_t flushes = 0, fulls = 0, runs = 0;
    for (uint32_t G : {8u, 16u})
        for (uint32_t nbins : bins)
            for (uint32_t ST : stages)
                for (uint32_t keep : keeps)
                    for (uint32_t r = 0; r < rounds; r++) {
                        const uint32_t seed = 977u * r + 31u * nbins + G + keep;
                        const uint32_t nw = r % 3 == 0 ? 1 : 8;
                        const uint32_t per_wave = r % 2 ? 3000 : (r == 0 ? 5 : 700); // r == 0: nothing but closing flushes
                        if (run(G, nbins, ST, keep, nw, per_wave, (int)(r % 3), seed, flushes, fulls)) return 1;
                        runs++;
                    }
    printf("runs=%llu flushes=%llu full=%llu ok\n", (unsigned long long)runs, (unsigned long long)flushes, (unsigned long long)fulls);
    return 0;
}
