// fora_consts.h -- the plain numbers that both the kernels (fora_kernels.h, fora_team.h) and the host-side table builders
// (fora_tables.h) and call planners (fora_rows.h, fora_seeds_plan.h, fora_sweep_plan.h) read.  No HIP: a plain C++ compiler
// takes this file.
#pragma once
#include <stdint.h>

namespace fora {

constexpr uint64_t FIX_ONE = 1ull << 62; // 1.0 of a ppr / residue word, and of a seed's weight

constexpr uint32_t DEG_SAT = 0xFFFFFFu; // rowinfo low 24 bits: out-degree, saturating
// bucketed push (graphs of up to MAX_BINS * BIN_SIZE nodes): increments are binned by target
// range and reduced in LDS instead of one global atomic per edge
#ifndef FORA_BIN_SHIFT
#define FORA_BIN_SHIFT 13
#endif
constexpr int BIN_SHIFT = FORA_BIN_SHIFT;      // narrow layout
constexpr uint32_t BIN_SIZE = 1u << BIN_SHIFT; // 8192 nodes -> 64 KiB of u64 accumulators in LDS
// Wide layouts: 16384-node bins (128 KiB of accumulators, one 1024-thread accumulate workgroup per CU): half the bins, so
// twice the messages per (chunk, bin) run, and a Twitter-2010-sized graph (2543 bins) needs ONE bin pass per level instead
// of two.  Same run: LJ-sized 280 indexed queries 904 -> 833 ms, Twitter-2010-sized 15.96 -> 18.48 q/s.
#ifndef FORA_BIN_SHIFT_WIDE
#define FORA_BIN_SHIFT_WIDE 14
#endif
constexpr int BIN_SHIFT_WIDE = FORA_BIN_SHIFT_WIDE;
constexpr uint32_t BIN_SIZE_WIDE = 1u << BIN_SHIFT_WIDE;
constexpr int MAX_BINS = 128;       // narrow layout: 4-B push messages, staged walk results
constexpr int MAX_BINS_WIDE = 1024; // wide layout: 8-byte messages (local target | value << 14), up to 1024 bins per pass ...
constexpr int MAX_BINS_HUGE = 2560; // ... or 2560 for graphs with more bins (Twitter-2010: 2543 bins, one pass)
constexpr int SEG_BITS = 32 - BIN_SHIFT; // narrow push message = (target & (BIN_SIZE-1)) << SEG_BITS | frontier position

// k_walk_dg: the tile of walk items that ticket k of workgroup x names.  A slot's tiles are dealt to its `sub` workgroups
// of nw waves as a static stride would deal them to the waves (wave w of workgroup x: x * nw + w, + tstride, ... with
// tstride = sub * nw); a workgroup hands ITS tiles out in ascending order, one ticket per tile, to the wave that asks.
// Ascending in k, so the first ticket at or past the slot's tile count ends the hand-out.
constexpr uint32_t dg_ticket_tile(uint32_t x, uint32_t nw, uint32_t tstride, uint32_t k) {
    return x * nw + k % nw + k / nw * tstride;
}

constexpr int SP_TILE = 512; // k_sparse_count / k_sparse_write: ids per workgroup and step, two per lane (fora_rows.h sizes their grid by it)
constexpr int SC_TILE = 512; // k_seed_combine: ids per workgroup and step, two per lane (fora_seeds_plan.h sizes its grid by it)

// team push (fora_team.h)
constexpr int TEAM_MAX = 32;                  // members of a team (5 bits of a target word)
constexpr int TEAM_LBITS = 15;                // bits of a local id
#ifndef FORA_TEAM_THREADS
#define FORA_TEAM_THREADS 1024
#endif
#ifndef FORA_TEAM_WGS_PER_CU
#define FORA_TEAM_WGS_PER_CU (FORA_TEAM_THREADS == 1024 ? 1 : 2)
#endif
constexpr int TEAM_WGS_PER_CU = FORA_TEAM_WGS_PER_CU;
constexpr uint32_t TEAM_R_CAP = TEAM_WGS_PER_CU == 1 ? 15296 : 7680; // local ids per member at most: 8 * (R + 1) + the static LDS of k_push_team <= 160 KiB / workgroups per CU
constexpr uint32_t TEAM_LMASK = (1u << TEAM_LBITS) - 1u;
constexpr uint32_t TEAM_EMPTY = 0xFFFFFFFFu;

} // namespace fora
