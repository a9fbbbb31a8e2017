// walk_dg_tickets_check.cpp -- the hand-out of a slot's tiles to the waves of k_walk_dg (fora_consts.h: dg_ticket_tile),
// restated on the CPU the way the kernel uses it: every workgroup of a slot keeps one ticket counter, a wave that needs a
// tile takes the next ticket, and a wave whose ticket names a tile at or past the slot's tile count takes no further one.
// For every item count and shape: the waves of all workgroups together visit every tile exactly once, whichever wave asks
// when; a workgroup's tickets name ascending tiles (so the first one past the end ends the hand-out, and the at most nw
// tickets taken after it are past the end too); and a workgroup visits exactly the tiles that a static stride gave its
// waves.  Built with -fsanitize=address,undefined by tests/test_walk_dg_tickets_cpu.py.
#include "fora_consts.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using fora::dg_ticket_tile;

static_assert(dg_ticket_tile(0, 8, 128, 0) == 0 && dg_ticket_tile(3, 8, 128, 7) == 31 && dg_ticket_tile(3, 8, 128, 8) == 152,
              "ticket k of workgroup x: tile x * nw + k % nw + k / nw * tstride");

#define CHECK(c) do { if (!(c)) { printf("line %d: %s (sub=%u nw=%u wt=%u nitems=%u)\n", __LINE__, #c, sub, nw, wt, nitems); return 1; } } while (0)

static int check(uint32_t sub, uint32_t nw, uint32_t wt, uint32_t nitems, uint32_t &rng, uint64_t &tickets) {
    const uint32_t ntiles = (nitems + wt - 1) / wt, tstride = sub * nw;
    std::vector<uint8_t> seen(ntiles, 0);   // an index at or past ntiles is the sanitizer's to catch
    std::vector<uint8_t> more(nw);
    for (uint32_t x = 0; x < sub; x++) {
        std::vector<uint8_t> mine(ntiles, 0); // the tiles of workgroup x under the static stride
        for (uint32_t w = 0; w < nw; w++)
            for (uint32_t t = x * nw + w; t < ntiles; t += tstride) mine[t] = 1;
        uint32_t ticket = 0, last = 0, left = nw; // the workgroup's counter; waves still asking
        more.assign(nw, 1);
        while (left) {
            rng = rng * 1664525u + 1013904223u; // which wave runs out of walks next: any order
            uint32_t w = (rng >> 16) % nw;
            while (!more[w]) w = (w + 1) % nw;
            const uint32_t k = ticket++;
            const uint32_t tile = dg_ticket_tile(x, nw, tstride, k);
            CHECK(k == 0 || tile > last);
            last = tile;
            if (tile >= ntiles) { more[w] = 0; left--; continue; }
            CHECK(left == nw);                // nobody had been sent away while a tile was left
            CHECK(mine[tile] == 1 && seen[tile] == 0);
            seen[tile] = 1;
            mine[tile] = 0;
        }
        CHECK(ticket <= ntiles / sub + 2 * nw); // a workgroup's share and one refusal per wave
        for (uint32_t t = 0; t < ntiles; t++) CHECK(mine[t] == 0);
        tickets += ticket;
    }
    for (uint32_t t = 0; t < ntiles; t++) CHECK(seen[t] == 1);
    return 0;
}

int main(int argc, char **argv) {
    const uint32_t max_items = argc > 1 ? (uint32_t)atoi(argv[1]) : 5000;
    // (workgroups per slot, waves per workgroup, items per tile): the kernel's shape, one workgroup per slot (option xb = 1),
    // half tiles, 16-wave workgroups, and shapes that are no powers of two
    const uint32_t shapes[][3] = {{16, 8, 32}, {1, 8, 32}, {16, 8, 16}, {1, 8, 16}, {2, 16, 32}, {1, 16, 64}, {3, 5, 7}, {1, 1, 1}, {7, 3, 64}};
    uint32_t rng = 12345;
    uint64_t tickets = 0;
    for (const auto &s : shapes)
        for (uint32_t nitems = 0; nitems <= max_items; nitems++)
            if (check(s[0], s[1], s[2], nitems, rng, tickets)) return 1;
    printf("shapes=%zu max_items=%u tickets=%llu ok\n", sizeof(shapes) / sizeof(shapes[0]), max_items, (unsigned long long)tickets);
    return 0;
}
