// fora_hip.hip -- C ABI (include/fora_hip.h) over the gfx950 kernels of fora_kernels.h.
//
// Owns all device state of one GPU: the CSR graph, the optional walk index, and a
// workspace of `batch` query slots.  The host side only sequences kernel launches;
// there is no CPU fallback: without a HIP device every entry point fails.
#include "fora_kernels.h"
#include "fora_topk_plan.h"
#include "fora_sparse_topk.h"
#include "fora_team.h"
#include "fora_bwd.h"
#include "fora_sweep.h"
#include "fora_tables.h"
#include "fora_rows.h"
#include "fora_seeds_plan.h"
#include "fora_prop.h"
#include "fora_propt.h"
#include "fora_sddmm.h"
#include "fora_softmax.h"
#include "fora_attn.h"
#include "fora_attn_bwd.h"
#include "fora_store.h"
#include "fora_cols.h"
#include "fora_subgraph.h"
#include "fora_subgraph_prop.h"
#include "../../include/fora_hip_gnn.h"

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

using namespace fora;

namespace {

// What an event pair times, named after the fora_timing field it feeds.  The switch of ev_collect is the one place that says which
// launches count under which kind.
enum EvKind { EV_PUSH_POP, EV_PUSH_EXPAND, EV_WALK_ALLOC, EV_WALK, EV_OTHER, EV_BATCH, EV_PUSH_ACCUM, EV_WALK_ACCUM, EV_ROUND_SWEEP,
              EV_PUSH_TAIL, EV_PUSH_TEAM, EV_BWD, EV_COMBINE, EV_SP_COMPACT, EV_SEED_COMBINE,
              EV_SW_COMPACT, EV_SW_SORT, EV_SW_CUT, EV_PROP_GATHER, EV_PROP_COMBINE, EV_PROPT_TRANSPOSE, EV_TK_SELECT, EV_SDDMM, EV_SOFTMAX, EV_ATTN, EV_STORE, EV_COLS, EV_SUB,
              EV_SUBP_T, EV_SUBP_SHORT, EV_SUBP_LONG };
struct EvPair { hipEvent_t a, b; EvKind kind; };

} // namespace

// Knobs of the engine.  Read ONCE per context (fora_hip_create: environment FORA_HIP_<NAME>, upper case) and changed
// afterwards only through fora_hip_set_option; nothing on a query path calls getenv.
struct Tunables {
    int64_t direct = 0;          // 1: the one-atomic-per-edge push (test reference)
    int64_t force_wide = 0;      // 1: wide bucket layout on small graphs too (tests)
    int64_t pass_bins = 0;       // bins handled per pass in the wide layout (0: by graph size)
    int64_t no_split = 0;        // 1: multi-pass graphs without the row-sorted copy / split offsets (tests)
    int64_t no_compact = 0;      // 1: no bit-packed walk copy (set_graph)
    int64_t walk_dg = 2;         // online walks over the degree-grouped copy (k_walk_dg): 0 never, 1 with one gather per walk for the endpoint's id, 2 results in bucket order; read by set_graph and at launch
    int64_t hubs = -1;           // (-1: 1024, or 4096 when the team push is this graph's default -- then the bin kernel does not run and the only reader of the hub copy is k_push_tail: 5.48 -> 4.89 ms per 1000 ws queries) narrow layout: increments for the `hubs` nodes of largest in-degree are summed per workgroup in LDS (Dev::col_hub); 0: off; read by set_graph.  ws, push of 1000 queries: 0 -> 79.5 ms, 1024 -> 75.6, 2048 -> 83.2, 4096 -> 90.5 (the LDS table costs the bin kernel its occupancy; the accumulate is bound by its sweep, not by its messages)
    int64_t hubs_wide = -1;      // the same for graphs that run the wide layout in one pass per level; -1: 2048 up to 2^28 edges, else 0 (off); read by set_graph.
                                 // LJ-sized push of 280 queries: 0 -> 560.8 ms, 1024 -> 558.7, 2048 -> 550.6, 4096 -> 681.6; Twitter-2010-sized: no gain (the top 2048 of 41.6 M nodes receive few of the edges)
    int64_t hub_min = 4096;      // ... in levels whose frontier holds at least this many nodes of the slot
    int64_t walk_flush_align = DG_FLUSH_ALIGN; // k_walk_dg: a flush of a wave's result stage stores whole aligned lines of this many results per bin and keeps the rest (stage_flush<.., G>, fora_flush_plan.h): 0 every flush sends all it holds, 8 lines of 64 bytes, 16 of 128.  Same bits for every value.  DESIGN.md 5.3 has the runs behind the default
    int64_t walk_flush_keep = 0; // ... results a wave's stage may keep at most (0: half the stage); a flush that would keep more sends everything.  Same bits for every value
    int64_t dg_hubs = 0;         // hub records of that copy (0: the fewest that leave <= 255 degree classes); read by set_graph
    int64_t bkcap = 0;           // bucket capacity in messages (0: default per layout)
    int64_t ovcap = 0;           // overflow list capacity (0: scales with the graph)
    int64_t tiny = 512;          // k_accum: buckets up to this many messages go by direct atomics
    int64_t xb = 0, ax = 0, wx = 0; // workgroups per slot: bin kernel / slab sweeps / walks (0: from the slot count)
    int64_t tail = -1;           // frontier size (largest slot) from which k_push_tail takes over (0: never, -1: by slot count)
    int64_t tail_always = 0;     // 1: do not wait for the frontier to have been large first (tests)
    int64_t select_compact = -1; // top-k select over compacted non-zeros: -1 by graph size, 0 never, 1 always
    int64_t rounds = 1;          // threshold rounds of the bucketed push (k_round_sweep): 2^(rounds-1) x the threshold first; 1: plain.
                                 // 2 rounds relax 17 % fewer edges (ws) but need 99 instead of 61 level launches: push 88 -> 126 ms per 1000 queries
    int64_t round_div = 4;       // leave a threshold round once the frontier is down to 1/round_div of the round's largest (0: when it is empty)
    int64_t defer = 0;           // bounded deferral of the bucketed push (Dev::defer_k): a node that crosses with less than 2^defer x its threshold waits one level; 0 (default): plain levels.
                                 // CHANGES THE SCHEDULE (like rounds / round_div): results equal the twin run with the same value (orc_twin_set_defer).
                                 // ws, 1000 queries, defer 1: 13.5 % fewer relaxations and 6 % fewer walks, but 22-32 instead of 19 level launches and a longer tail: push 75 -> 99-114 ms
    int64_t defer_min = 0;       // with defer: only levels that pop at least this many nodes of the slot defer (orc_twin_set_defer_min)
    int64_t team = -1;           // graphs of the narrow layout push with k_push_team (a slot's residue resident in the LDS of a team of workgroups, fora_team.h): 0 never (the bucketed
                                 // kernels), 1 / -1 (default) always.  Same bits either way.  Measured, push of 1000 queries (round 6): ws-sized graph 45.7 + 4.9 ms against 77.8 bucketed; R-MAT
                                 // variant with 52 % dangling nodes (483 sources with out-edges) 24.3 + 5.4 against 41.5 (round 4: 47.3 against 41.3, hence a gate on the dangling share until round 6)
    int64_t team_size = 0;       // members per team (a power of two up to 32); 0: the fewest whose LDS holds the graph; read by set_graph
    int64_t team_tail = -1;      // frontier size (of a slot) at which k_push_team hands the slot to k_push_tail; 0: never; -1: 4096
    int64_t team_xcd = 1;        // 1: the members of a team share blockIdx % 8 (one XCD under round-robin placement: speed only)
    int64_t team_max = 0;        // teams per launch at most (0: one member per CU); tests
    int64_t team_hubs = 1024;    // k_push_team: increments for the nodes of largest in-degree are summed per member in LDS, one message per hub and level (0: off); read when the team tables are built
    int64_t tail_hubs = 1;       // k_push_tail: increments for the hubs of the hub copy are summed in LDS (0: every relaxation is an atomic)
    int64_t team_log = -1;       // k_push_team: entries of a member's reserve log per slot (-1: 2^17; 0: none, every pop adds to its accumulator; tests use small values for the mixed case)
    int64_t slot_major = -1;     // wide layouts: which launches put the slot in blockIdx.x (Dev::slot_major; bits 1 bin kernel, 2 accumulate, 4 indexed walks, 8 walk allocation); -1: by call type and slot count (make_dev); 0: round 5's order
    int64_t acc_group = 0;       // wide accumulate: bins per workgroup (0: by the launch's size, 1 ... 8; tests force 1 / 3 / 16)
    int64_t team_abort_level = 0; // tests: every team abandons its launch (as after a time-out) when a slot reaches this level -- an abort in mid-flight: partial slabs, logs, message buffers, tagged words
    int64_t team_timeout_ms = 500; // k_push_team: a member that has waited this long for its team gives up; the call then runs again through the bucketed kernels (with_retry)
    int64_t team_coop = 0;       // k_push_team launch: 0 (default) plain launch behind an occupancy check (occupancy x CUs >= grid, team_fits); 1: hipLaunchCooperativeKernel.  Measured on ROCm 7.2 / MI355X (round 5): the cooperative
                                 // launch costs ~9 ms per launch (push of 64 ws-sized queries 14.8 ms against 5.6: the runtime moves the launch to its cooperative queue and back) and a process with two contexts that used it crashed in the runtime's teardown -- opt-in only
    int64_t topk_bk_div = 16;    // top-k (--opt driver) on wide graphs: message buckets of 1 / this of a query's capacity (plan_workspace); 1: as large as a query's.
                                 // Twitter-2010-sized, k = 500 --opt --with_idx, 125 sources: 1 -> 245 q/s (8 slots per batch), 8 -> 279 (30), 16 -> 303 (37), 32 -> 304 (41), 64 -> 306 (44); same bits
    int64_t quads = 1;           // wide layouts, one bin pass per level: k_pushq_bin reads quad-padded copies of col / col_hub with 16-byte loads (0: single edges, round 4)
    int64_t profile = 1;         // 0: no HIP event pairs around the launches
    int64_t grid = 2048;         // workgroups of the direct-path kernels
    int64_t bwd_lds_cap = BWD_CAP_DEFAULT; // backward push: entries per target's LDS table (at most BWD_CAP_MAX); a target with more goes to the global tier; 0: every target does
    int64_t bwd_chunk = 0;       // backward push: targets per chunk (0: as many as the entry budget from free HBM holds)
    int64_t tgt_lanes = -1;      // targeted BiPPR combine (k_bippr_combine_targets): 0 lane = slot over the transposed walk slabs, 1 lane = entry over the slot-major ones, -1: by the batch's slots and the call's entries (want_by_slot).  Same bits either way
    int64_t tgt_span = 0;        // ... entries per wave (0: from the chunk's entries, 64 .. 1024).  Same bits for every value
    int64_t sweep_lds_cap = SW_TILE_MAX; // sweep cut (fora_hip_sweep_batch): entries of a sort tile, rounded down to a power of two (at most SW_TILE_MAX); a row that fits one is sorted by one workgroup in LDS, a longer one takes the global tier; 0: every row does, every step in global memory.  Same bits for every value
    int64_t sweep_rows = 0;      // ... rows whose rank maps are live at a time (the rank block holds that many slabs of n words); 0: 256.  Same bits for every value
    int64_t seeds_dedup = 1;     // seed sets (fora_hip_query_seeds_batch): 1 a seed id runs once per call whatever the number of sets that list it; 0 every listed seed takes a slot of its own (tests, tools/seeds_bench.py).  Same bits either way
    int64_t prop_segs = 0;       // PROPAGATE (fora_hip_sparse_propagate): segments whose partial sums are live at a time (a chunk of the call; the partial-sum buffer holds that many rows of d doubles); 0: by free memory, otherwise at least 1.  Same bits for every value
    int64_t propt_lds_cap = PROPT_LDS_MAX; // PROPAGATE, TRANSPOSED (fora_hip_sparse_propagate_t): keys of a column's run that one workgroup sorts in LDS at most (clamped to 0 .. PROPT_LDS_MAX); a longer run takes the global tier, one of at most 64 keys a wave; 0: every run of two keys or more takes the global tier.  Same bits for every value; a change drops the cached transposition
    int64_t topk_lds_cap = TOPK_LDS_MAX; // SPARSE RESULTS, TOP-K (fora_hip_query_sparse_topk_batch, fora_hip_seeds_sparse_topk_batch): candidates of a cut row that one workgroup stages in LDS at most (clamped to 0 .. TOPK_LDS_MAX, fora_topk_plan.h); a longer row is selected from global memory; 0: every cut row is.  Same bits for every value
    int64_t topk_cand = 0;       // ... entries of the candidate scratch (the rows of a batch are compacted into it chunk by chunk, consecutive rows, a row never split); 0: by free memory; always at least the longest row.  Same bits for every value
    int64_t softmax_short = SMAX_SHORT_MAX; // ROW SOFTMAX (fora_hip_sparse_softmax, fora_hip_sparse_softmax_bwd): a row of at most this many entries (clamped to 0 .. 256, fora_softmax.h) is one wave's, read once and written once; a longer one goes segment by segment through partial maxima and sums; 0: every row does.  Same bits for every value
    int64_t attn_short = ATTN_SHORT_MAX; // ATTENTION (fora_hip_sparse_attention): a non-empty row of at most this many entries (clamped to 0 .. 256, fora_attn_plan.h) is one wave's per head in the fused kernel k_attn_short; a longer one goes through the kernels of SCORES, ROW SOFTMAX and PROPAGATE WITH VALUES inside the same call; 0: every row does.  Same bits for every value.  ATTENTION, BACKWARD (fora_hip_sparse_attention_bwd) reads it for rows (k_attn_bwd_short) and columns (k_attn_cols, fora_attn_bwd_plan.h) alike
    int64_t take_span = STORE_SPAN_DEFAULT; // ROW STORE (fora_hip_store_take; the check of fora_hip_store_load): output entries one workgroup copies, a multiple of 64 and at least 64 (store_span, fora_store_plan.h).  Same bits for every value.  DESIGN.md 5.20 has the runs behind the default
    int64_t cols_block = COLS_BLOCK_DEFAULT; // COLUMNS (fora_hip_sparse_compact): words of the bitmap one workgroup of k_cols_totals / k_cols_list counts, a power of two from 1 to 4096 (cols_block, fora_cols_plan.h).  Same bits for every value.  DESIGN.md 5.21 has the runs behind the default
    int64_t sub_span = SUB_SPAN_DEFAULT; // SUBGRAPH (fora_hip_sparse_subgraph): scanned edges one workgroup of k_sub_count / k_sub_write takes, a power of two from 256 to 8192 (sub_span, fora_subgraph_plan.h).  Same bits for every value.  The default is provisional and unmeasured
    int64_t sub_short = SUB_SHORT_DEFAULT; // SUBGRAPH PRODUCTS (fora_hip_subgraph_propagate, fora_hip_subgraph_propagate_t): an output row of at most this many entries (clamped to 0 .. 256, fora_subgraph_prop_plan.h) is summed and written by the one-pass kernel k_sub_agg; a longer one goes through the kernels of PROPAGATE inside the same call; 0: every non-empty row does.  Same bits for every value
    int64_t seeds_rows = 256;    // seed sets, sparse rows and sweeps (fora_hip_seeds_sparse_batch, fora_hip_seeds_sweep_batch): rows of the accumulator block compacted / sorted at a time (at least 1; seeds_chunk); bounds the count, total, descriptor and sort buffers.  Same bits for every value
};
static const struct { const char *name; int64_t Tunables::*field; bool layout; } OPTIONS[] = {
    {"direct", &Tunables::direct, true}, {"force_wide", &Tunables::force_wide, true}, {"pass_bins", &Tunables::pass_bins, true},
    {"no_split", &Tunables::no_split, true}, {"no_compact", &Tunables::no_compact, false}, {"walk_dg", &Tunables::walk_dg, false}, {"walk_flush_align", &Tunables::walk_flush_align, false}, {"walk_flush_keep", &Tunables::walk_flush_keep, false}, {"dg_hubs", &Tunables::dg_hubs, false}, {"hubs", &Tunables::hubs, true}, {"hubs_wide", &Tunables::hubs_wide, true}, {"hub_min", &Tunables::hub_min, false}, {"bkcap", &Tunables::bkcap, true},
    {"ovcap", &Tunables::ovcap, true}, {"tiny", &Tunables::tiny, false}, {"xb", &Tunables::xb, false}, {"ax", &Tunables::ax, false},
    {"wx", &Tunables::wx, false}, {"tail", &Tunables::tail, false}, {"tail_always", &Tunables::tail_always, false},
    {"select_compact", &Tunables::select_compact, false}, {"team", &Tunables::team, true}, {"team_size", &Tunables::team_size, true}, {"team_tail", &Tunables::team_tail, false}, {"team_xcd", &Tunables::team_xcd, false}, {"team_max", &Tunables::team_max, true}, {"team_hubs", &Tunables::team_hubs, true}, {"team_log", &Tunables::team_log, false}, {"topk_bk_div", &Tunables::topk_bk_div, true}, {"quads", &Tunables::quads, false}, {"team_timeout_ms", &Tunables::team_timeout_ms, false}, {"team_abort_level", &Tunables::team_abort_level, false}, {"acc_group", &Tunables::acc_group, false}, {"slot_major", &Tunables::slot_major, false}, {"team_coop", &Tunables::team_coop, false}, {"tail_hubs", &Tunables::tail_hubs, false}, {"rounds", &Tunables::rounds, false}, {"defer", &Tunables::defer, true}, {"defer_min", &Tunables::defer_min, false}, {"round_div", &Tunables::round_div, false},
    {"profile", &Tunables::profile, false}, {"grid", &Tunables::grid, false},
    {"bwd_lds_cap", &Tunables::bwd_lds_cap, false}, {"bwd_chunk", &Tunables::bwd_chunk, false},
    {"tgt_lanes", &Tunables::tgt_lanes, false}, {"tgt_span", &Tunables::tgt_span, false},
    {"seeds_dedup", &Tunables::seeds_dedup, false}, {"seeds_rows", &Tunables::seeds_rows, false},
    {"sweep_lds_cap", &Tunables::sweep_lds_cap, false}, {"sweep_rows", &Tunables::sweep_rows, false},
    {"prop_segs", &Tunables::prop_segs, false}, {"propt_lds_cap", &Tunables::propt_lds_cap, false},
    {"topk_lds_cap", &Tunables::topk_lds_cap, false}, {"topk_cand", &Tunables::topk_cand, false},
    {"softmax_short", &Tunables::softmax_short, false}, {"attn_short", &Tunables::attn_short, false},
    {"take_span", &Tunables::take_span, false}, {"cols_block", &Tunables::cols_block, false}, {"sub_span", &Tunables::sub_span, false},
    {"sub_short", &Tunables::sub_short, false},
};
// knobs that choose another push SCHEDULE (other, equally valid result bits): never taken from the environment -- a stray
// variable must not change what a query returns; fora_hip_set_option sets them (tests, experiments)
static bool schedule_option(const char *name) {
    return !strcmp(name, "rounds") || !strcmp(name, "round_div") || !strcmp(name, "defer") || !strcmp(name, "defer_min");
}
static Tunables tunables_from_env() {
    Tunables t;
    for (const auto &o : OPTIONS) {
        if (schedule_option(o.name)) continue;
        std::string env = "FORA_HIP_";
        for (const char *p = o.name; *p; p++) env += (char)toupper((unsigned char)*p);
        if (const char *e = getenv(env.c_str())) if (*e) t.*(o.field) = atoll(e);
    }
    return t;
}

// Owning device (PINNED: pinned host) buffer of `count` elements, move-only.  The size is written once, at alloc(); the
// clears take it from the buffer, and a clear or a part beyond it is an error instead of a write out of bounds.
template <typename T, bool PINNED = false> class DevBuf {
    T *p = nullptr;
    size_t count = 0;
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), count(o.count) { o.p = nullptr; o.count = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); std::swap(p, o.p); std::swap(count, o.count); } return *this; }
    ~DevBuf() { reset(); }
    void reset() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; count = 0; }
    hipError_t alloc(size_t cnt) { // frees what it held; holds nothing after a failure
        reset();
        const hipError_t e = PINNED ? hipHostMalloc((void **)&p, cnt * sizeof(T)) : hipMalloc((void **)&p, cnt * sizeof(T));
        if (e == hipSuccess) count = cnt; else p = nullptr;
        return e;
    }
    hipError_t ensure(size_t cnt) { return p && count >= cnt ? hipSuccess : alloc(cnt); }
    hipError_t upload(const T *src, size_t cnt, size_t min_count = 0) { // alloc(cnt, or min_count if that is more) + a blocking copy of cnt elements from the host; holds nothing after a failure
        hipError_t e = alloc(std::max(cnt, min_count));
        if (e == hipSuccess && cnt) e = hipMemcpy(p, src, cnt * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) reset();
        return e;
    }
    hipError_t upload(const std::vector<T> &v, size_t min_count = 0) { return upload(v.data(), v.size(), min_count); }
    hipError_t fill(hipStream_t s, int byte, size_t from, size_t cnt) const { // elements [from, from + cnt)
        return from + cnt > count ? hipErrorInvalidValue : hipMemsetAsync(p + from, byte, cnt * sizeof(T), s);
    }
    hipError_t zero(hipStream_t s) const { return fill(s, 0, 0, count); }
    hipError_t zero(hipStream_t s, size_t cnt) const { return fill(s, 0, 0, cnt); } // a prefix
    T *part(size_t i, size_t stride) const { return p ? p + i * stride : nullptr; } // i-th of equal parts (the parity pairs); null when empty
    T *get() const { return p; }
    size_t size() const { return count; }
    explicit operator bool() const { return p != nullptr; }
};
template <typename T> using PinBuf = DevBuf<T, true>;

// What a workspace is sized for (plan_workspace): the one copy of these words.  Every reader goes through Workspace::plan.
struct WsPlan {
    bool binned = false;                // bucketed push; false: the one-atomic-per-edge path (option `direct`)
    int nbins = 0, pbins = 0;           // bins of the graph; bins per pass (bucket-array stride)
    uint32_t sub = 0, bk_cap = 0;       // sub-buckets per (slot, bin) = producer workgroups per slot; capacity of one sub-bucket
    uint32_t ov_cap = 0, dbm_words = 0; // per slot: entries of the bucket-overflow list, words of the deferral bitmap
    uint64_t segq_cap = 0, wit_cap = 0; // per slot: frontier positions, walk items
    uint64_t wl_cap = 0, seg_cap = 0;   // all slots: entries of a slab, PushSeg entries of the scratch
    uint32_t team_rlog_cap = 0;         // entries of a member's reserve log per slot (Workspace::d_team_rlog_id): follows from the memory that is free when
                                        // the team buffers are allocated, so ensure_workspace writes it there, not plan_workspace
    uint64_t segs = 0, scratch = 0, per_slot = 0; // planning intermediates, per slot: PushSeg entries, scratch bytes, bytes in all
    bool fits(const WsPlan &want) const { // can buffers sized for this plan serve a call that plans `want` for the same slot count?
        return binned == want.binned && pbins == want.pbins && seg_cap >= want.seg_cap && wit_cap >= want.wit_cap && bk_cap == want.bk_cap && sub == want.sub;
    }
};

// Everything that lives and dies with one plan of the query slots (ensure_workspace; the lazily allocated members: their
// first user), the plan included.  free_workspace assigns a fresh one: the initialisers below are the reset values.  ensure_workspace builds
// into a local value and moves it in after its last step: the workspace is complete or empty (B == 0, an empty plan), never half-built.
struct Workspace {
    int B = 0, B_memcap = 0; // slots; slots that fitted the free memory when the workspace was planned (>= B)
    WsPlan plan;
    DevBuf<uint64_t> d_residue, d_ppr, d_wl[2];
    DevBuf<unsigned char> d_scratch; // PushSeg list during the push, WalkItem list during the walks
    DevBuf<unsigned long long> d_counters; // wl_count | seg_count | wit_count | tot_steps
    DevBuf<QState> d_qs; DevBuf<int32_t> d_src; DevBuf<uint32_t> d_err;
    // bucketed push (n <= MAX_BINS * BIN_SIZE)
    DevBuf<uint32_t> d_fl[2], d_fl_count; DevBuf<uint64_t> d_inc_tab[2]; // fl_count: [2][B * CSTRIDE]
    DevBuf<uint32_t> d_ov_w, d_ov_count, d_ov_bin; DevBuf<uint64_t> d_ov_inc; // bucket overflow list, its size [2][B * CSTRIDE], its entries per bin [2][B][nbins]
    DevBuf<uint32_t> d_bk_w, d_bk_count; DevBuf<uint64_t> d_bk_inc; // bk_w: empty in the wide layout
    DevBuf<uint32_t> d_wit_count; // [B * CSTRIDE]
    DevBuf<uint32_t> d_sw;        // [2][B * CSTRIDE] k_round_sweep: append counters, finished-workgroup tickets
    DevBuf<uint32_t> d_tile_ctr;  // [2][B * CSTRIDE] wide bin kernels: next tile of a slot (Dev::tile_ctr)
    DevBuf<uint64_t> d_dbm;       // [2][B][dbm_words] bounded deferral: marks of the deferred nodes (Dev::dbm)
    DevBuf<uint32_t> d_dflag;     // [2][B][nbins]
    DevBuf<uint32_t> d_dl;        // [2][B][n] k_push_tail's deferred lists; empty without the `defer` option
    DevBuf<uint64_t> d_hubsum;    // [B][sub][hubs]; empty: no hub pre-aggregation
    PinBuf<uint32_t> h_flc;       // pinned ring of per-slot frontier sizes
    // team push (fora_team.h); d_team_msg empty: no team push with this workspace
    DevBuf<uint32_t> d_team_msg;
    DevBuf<uint64_t> d_team_inct, d_team_rsvl; // rsvl: reserve accumulators by local id
    DevBuf<uint16_t> d_team_rlog_id; DevBuf<uint64_t> d_team_rlog_val; // reserve logs (TeamDev::rlog_id)
    DevBuf<unsigned long long> d_team_cnt; // the teams' barrier words (TeamDev::cntw)
    DevBuf<uint32_t> d_team_ctl;           // team_ctl_layout
    uint32_t team_n = 0;                   // teams of a launch
    int team_fit = -1;                     // 1: every workgroup of a k_push_team launch fits the device at once (occupancy x CUs >= grid); 0: no team push; -1: not asked yet
    // allocated by their first user (ensure(): each on its own)
    DevBuf<uint64_t> d_ppr2, d_cursor; // top-k: per-round ppr, index cursors (rw_counter)
    uint32_t cursor_epoch = 0;         // batch serial number stamped into the cursor words (k_walk_alloc): 0 = the slabs hold no valid word
    DevBuf<uint8_t> d_active; DevBuf<unsigned long long> d_above;
    DevBuf<double> d_sel_thr; // [B] launch_select: per-slot limit of the entries that can be among the top k
    // top-k with bounds: upper_bounds / lower_bounds (query.h:1350-1353), topk_filter marks, stop flags, walks of the round
    DevBuf<double> d_upper, d_lower;
    DevBuf<uint8_t> d_filter; DevBuf<uint32_t> d_fail; DevBuf<unsigned long long> d_round_walks;
    DevBuf<uint32_t> d_nz_counts; // [B][NZ_X + 1]: per-block non-zero counts, then the slot's total
    DevBuf<int32_t> d_lb_ids, d_topk_ids; DevBuf<double> d_lb_sc, d_topk_sc; // (ids, scores) pairs of B * k entries
    PinBuf<unsigned long long> h_pinned; // [MAX_LEVELS + 2] frontier sizes read back
    PinBuf<QState> h_qs_pin;             // pinned landing area of the per-slot accumulators
    PinBuf<unsigned long long> h_steps_pin;
};

// The graph and everything derived from it (fora_hip_set_graph; the lazily built parts: their first user).  free_graph
// assigns a fresh one.  A part that is rebuilt on its own is a struct of its own and is complete or empty: its builder
// resets it, builds into a local value and moves that in after the last step has succeeded.
struct RowSplit { // multi-pass graphs: row-sorted copy of col (empty: the rows are sorted as loaded), split offsets [n][npass + 1]
    DevBuf<int32_t> d_col_push; DevBuf<uint32_t> d_row_split;
    int pbins = 0;
};
struct HubCopy { // hub pre-aggregation (Dev::col_hub)
    DevBuf<int32_t> d_col_hub; DevBuf<uint32_t> d_hub_node, d_hub_first;
    uint32_t hubs = 0;
    int shift = 0;         // bin shift the hub ranges were built for
    bool for_team = false; // sized for the team path (4096 hubs, k_push_tail its only reader); set without a copy too
};
struct QuadCopies { // quad-padded copies for the wide bin kernel (Dev::col4); empty: not built
    DevBuf<int32_t> d_col4, d_col_hub4; DevBuf<uint64_t> d_rowinfo4;
    uint64_t quads = 0;
};
struct WalkCopy { // degree-grouped walk copy: the arrays dg points into; dg.colp == nullptr: none
    DevBuf<uint32_t> d_perm, d_inv, d_colp, d_rec, d_invb; DevBuf<uint8_t> d_T;
    WalkDG dg{};
};
struct TeamTables { // team push (fora_team.h): target copy of col, bucket offsets; for graphs of the narrow layout
    DevBuf<uint32_t> d_colt, d_off, d_n2l, d_l2n, d_hubtgt;
    DevBuf<uint32_t> d_rowq;  // [n] first quad of every node's row in d_colt
    DevBuf<uint64_t> d_rowl;  // rows by local id
    DevBuf<uint16_t> d_deg16;
    uint32_t H = 0, T = 0, R = 0; // hubs, members per team, local ids per member; T == 0: this graph does not take the team path
    uint64_t cap = 0;             // message slots per (team, parity)
    bool checked = false, wanted = false; // ensure_team has looked at this graph with these options ...
    uint32_t force = 0, hubs_opt = 0;     // ... the team_size / team_hubs options among them
};
struct ReverseCsr { DevBuf<int64_t> d_rin_ptr; DevBuf<int32_t> d_rin; }; // backward push (fora_bwd.h), built on first use
struct GlobalTier { // backward push: [wgs][n] each, kept zero
    DevBuf<uint64_t> d_gr, d_gp, d_gfy; DevBuf<uint32_t> d_gtag, d_glist, d_gfn;
    uint32_t wgs = 0;
};
struct Graph {
    int32_t n = 0;
    int64_t m_attr = 0, nnz = 0;
    std::vector<int64_t> h_row_ptr;
    DevBuf<int64_t> d_row_ptr; DevBuf<int32_t> d_col; DevBuf<uint64_t> d_rowinfo; DevBuf<uint32_t> d_deg;
    DevBuf<uint32_t> d_rp32, d_colp; // compact walk copy
    uint32_t colbits = 0;
    double dangling_frac = 0; // share of the nodes without out-edges
    RowSplit split; HubCopy hub; QuadCopies quad; WalkCopy walk; TeamTables team; ReverseCsr rev; GlobalTier tier;
};
// Walk index (build_index / set_index; free_index, set_graph).
struct Index {
    DevBuf<int32_t> d_rw_idx; DevBuf<uint64_t> d_idx_off, d_idx_cnt;
    uint64_t len = 0;
    bool have = false;
};
// Backward push and BiPPR: buffers of their own, apart from the FORA workspace; grow-only, kept across graphs until destroy.
struct BwdBufs {
    DevBuf<int32_t> d_bt; // targets of the call
    DevBuf<uint32_t> d_bcnt, d_bspill, d_blist; DevBuf<uint8_t> d_bflag; DevBuf<uint64_t> d_boff;
    DevBuf<uint32_t> d_enode; DevBuf<uint64_t> d_ep, d_er; // entries of a chunk
    DevBuf<unsigned long long> d_bstat;
    // targeted BiPPR (fora_hip_bippr_targets_batch): the estimate block of a batch, slot-major [nb][nt] and then the nb row
    // sums; its f64 copy.  nt has nothing to do with n, so these are no slabs of the workspace
    DevBuf<uint64_t> d_tgt_est; DevBuf<double> d_tgt_f64;
};
// Seed sets (fora_hip_query_seeds_batch): buffers of their own, apart from the workspace; grow-only, kept until set_graph or destroy.
struct SeedBufs {
    DevBuf<uint64_t> d_acc;  // the accumulator block of a call, [ns][n] at 2^-62 (n changes with the graph: no slabs of the workspace's plan)
    DevBuf<uint64_t> d_list; // use list of the batch in progress (SeedBatch::pack, fora_seeds_plan.h); the dangling seeds' triples after the last batch
    DevBuf<unsigned long long> d_sums; // [ns] row sums
};
// A result over rows that stays on the device until it is fetched: the sparse rows and the sweep profiles.  Both lay their
// rows out in the caller's order (RowLayout, fora_rows.h), fill their held arrays batch by batch behind the same count pass
// (CountBufs, count_rows) and grow them by the same rule (reserve_rows); finish_rows writes the dangling rows' entries and
// marks the result held; every entry point that makes one first ends the held one (held_rows_begin).  Their own: below.
struct CountBufs { // count pass of the batch in progress
    DevBuf<uint32_t> d_counts, d_tot; // per workgroup [slots][X] and per slot
    PinBuf<uint32_t> h_tot;           // pinned landing area of d_tot
};
struct HeldRows {
    uint64_t entries = 0; bool valid = false; // valid: a result is held (it may have no entries)
    CountBufs cnt;
};
// Sparse result of the last fora_hip_query_sparse_batch (free_sparse: sparse_clear, set_graph), apart from the workspace --
// free_workspace (set_batch, set_option, a bucket retry) leaves it alone.
struct SparseResult : HeldRows {
    DevBuf<int32_t> d_ids; DevBuf<uint64_t> d_fix; // entries of all rows, rows in the caller's order
    DevBuf<int64_t> d_base;           // first entry of every live row of the call
    DevBuf<double> d_stage;           // fora_hip_sparse_fetch: vals on their way to a host array, SP_STAGE at a time
    // top-k rows (fora_sparse_topk.h): the candidate scratch, a CSR of (id, word) over the rows of the chunk in progress, and
    // the chunk's descriptors (the write bases of its rows, then its TopkRow lists)
    DevBuf<int32_t> d_cand_ids; DevBuf<uint64_t> d_cand_fix; DevBuf<uint64_t> d_tkdesc;
    // COLUMNS (fora_hip_sparse_compact): d_ids hold ranks in the result's own `cols` columns, not node ids.  A flag of its own:
    // cols == 0 is a legal compacted result.  Ends with the held result (sparse_unheld)
    bool compacted = false; uint64_t cols = 0;
};
// Sweep profile of the last fora_hip_sweep_batch (free_sweep: sweep_clear, set_graph), apart from the workspace and from the
// sparse result; the buffers of the call in progress live here too.
struct SweepResult : HeldRows {
    DevBuf<int32_t> d_ids; DevBuf<uint64_t> d_cut, d_vol; // profiles of all rows, rows in the caller's order
    DevBuf<int32_t> d_tids; DevBuf<uint64_t> d_tkey;          // padded (id, key) copies of the batch's rows: the sort buffers
    DevBuf<uint64_t> d_desc;                                  // descriptors of the batch: SweepRowDesc | base | SweepTile | SweepGRow
    DevBuf<SweepRowOut> d_out; PinBuf<SweepRowOut> h_out;     // per live row of the batch
    DevBuf<int32_t> d_rank;                                   // [rank_rows][n], -1 between uses
    uint32_t rank_rows = 0;
    bool rank_dirty = false; // a call ended between a scatter and its reset
};

// PROPAGATE (fora_hip_sparse_propagate): buffers of the call in progress, kept between calls and grown when a call needs more
// (free_prop: set_graph, destroy).  Apart from the sparse result they read.
struct PropBufs {
    // uploads of host operands, made on every call (HeldIn::stage names the buffer an operand goes to): the matrix with n rows
    // (feat, b, k); the one with nq rows (a, q; ROW SOFTMAX's grad); the per-entry vector (values, scores, y); v; g
    DevBuf<unsigned char> d_feat, d_a, d_vals, d_v, d_g;
    // outputs on their way to host arrays (HeldOut::reserve): the nq-row or per-entry output of every call (dq too); y; dk; dv
    DevBuf<float> d_out32, d_y32, d_dk32, d_dv32; DevBuf<double> d_out64, d_y64, d_dk64, d_dv64;
    // scratch of the launches
    DevBuf<PropSeg> d_segs; DevBuf<PropRowRec> d_recs;   // the call's plan (fora_prop_plan.h)
    DevBuf<double> d_part; DevBuf<uint64_t> d_segsum;    // partial sums [prop_segs][d] and word sums [prop_segs] of the chunk in progress
    DevBuf<double> d_carry; DevBuf<uint64_t> d_scarry;   // [2][d] / [2]: the row a chunk cut, one buffer read and one written per chunk
    DevBuf<double> d_smax; DevBuf<uint32_t> d_smax_nan;  // ROW SOFTMAX: [2][long segments] segment maxima and sums; [1] the rows written as NaN
    DevBuf<double> d_attn_s, d_attn_y;                   // ATTENTION: [entries] the scores (BACKWARD: dy) and the y of the longer rows, one head at a time
    DevBuf<double> d_attn_ds;                            // ATTENTION, BACKWARD: [heads][entries] ds, written by the row side and read by the column side
};
// PROPAGATE, TRANSPOSED (fora_hip_sparse_propagate_t, fora_hip_sparse_transpose_fetch): the transposition of the held sparse
// result, built by the first of the two calls after a result becomes held and kept with it -- it ends wherever the held
// result ends (sparse_unheld, free_sparse) and when the option "propt_lds_cap" changes.  Complete or empty: the builder fills
// a local value and moves it in after its last step.
struct PropTBufs {
    bool built = false;
    DevBuf<int32_t> d_rows; DevBuf<uint64_t> d_fix;      // [entries] the row and the held word of every entry, column by column
    DevBuf<int64_t> d_col_ptr; std::vector<int64_t> h_col_ptr; // [n + 1] and its host copy (the product is planned from it)
    DevBuf<uint64_t> d_rsum;                             // [nq] S_i, the wrapping sum of row i's words
    DevBuf<int64_t> d_pos; bool has_pos = false;         // [entries] the held place of every transposed entry: made by the first call with values (PROPAGATE WITH VALUES), never by a plain one
    int nq = 0;                                          // rows of the row_ptr it was built from
    uint64_t columns = 0, max_col = 0;
    uint32_t short_cols = 0, lds_cols = 0, global_cols = 0;
    // ATTENTION, BACKWARD: the split of the columns (fora_attn_bwd_plan.h), planned by the first call under a value of "attn_short"
    // and a chunk size, its lists resident on the device; it ends with the transposition, being a member of it
    struct ColPlan {
        bool valid = false;
        uint32_t short_cap = 0; uint64_t chunk_segs = 0, long_segs = 0; // the key, and the long columns' segments under that cap
        AttnColPlan plan;                                               // (host: the chunks of plan.lng sequence the launches)
        DevBuf<PropSeg> d_short, d_lsegs; DevBuf<PropRowRec> d_lrecs;
    } cols;
};

// ROW STORE (fora_hip_store_put, _load, _take, _info, _clear): a library of sparse rows 0 .. R - 1 kept on the device, apart from the
// workspace and from the held sparse result, until fora_hip_store_clear, set_graph or destroy (free_store).  row_ptr lives on the
// host: a take is planned from it, and the kernels read the plan.  d_ids / d_fix may have room behind `entries`: an append that
// fits is written there, and is part of the store only once the words below have moved.
struct RowStore {
    std::vector<int64_t> h_row_ptr;           // R + 1 (empty: no store, R = 0)
    DevBuf<int32_t> d_ids; DevBuf<uint64_t> d_fix;
    uint64_t entries = 0, max_row = 0;
    int64_t rows() const { return h_row_ptr.empty() ? 0 : (int64_t)h_row_ptr.size() - 1; }
    // scratch of the call in progress, grow-only: the plan (out_ptr | src | win, fora_store_plan.h); the check's smallest bad entry
    DevBuf<int64_t> d_plan; DevBuf<unsigned long long> d_bad;
};

// COLUMNS (fora_hip_sparse_compact, fora_hip_sparse_cols_fetch): the bitmap over the n nodes, the rank of every word's first set
// bit, the blocks' totals and offsets, nc, and U itself.  d_cols is U while the held result is compacted (SparseResult::cols
// entries of it), and d_bitmap and d_wrank describe U for as long: cols_compact_impl is their only writer, and a compacted result
// is not compacted again -- SUBGRAPH reads them.  The totals, offsets and nc are scratch of the call in progress.  Grow-only,
// freed by set_graph and destroy (free_cols).
struct ColsBufs {
    DevBuf<unsigned long long> d_bitmap, d_nc; DevBuf<uint32_t> d_wrank, d_btot; DevBuf<int32_t> d_cols;
};

// SUBGRAPH (fora_hip_sparse_subgraph, fora_hip_sparse_subgraph_fetch): the CSR the graph induces on the columns of the compacted
// held result -- d_ptr [nc + 1], d_col and d_eid [edges] while `valid` -- and the scratch of the call in progress: scan_ptr
// [nc + 1] and base [nc] of the rows, the row blocks' totals | offsets, the spans' kept counts and offsets, S | edges.  valid
// ends with the held result (sparse_unheld).  Grow-only, freed by set_graph and destroy (free_sub).
// SUBGRAPH PRODUCTS (include/fora_hip_gnn.h) keep what they derive from the held subgraph in `prop`: its transposition, built by
// the first transposed call or fora_hip_subgraph_transpose_fetch, and per side the host copy of the offsets with the plan of
// the long rows and its device tables, made by the first call that needs them under a value of "sub_short" and a chunk size.
// All of it ends when the subgraph ends or is built again (sub_prop_drop) and is freed by free_sub.
struct SubProp {
    struct Side {
        bool have_ptr = false; std::vector<int64_t> h_ptr;  // the offsets on the host: sub_ptr / in_ptr
        bool planned = false; uint32_t cap = 0; uint64_t per = 0; // the key of the plan
        SubSplit split; PropPlan plan;                      // (host: the chunks sequence the launches)
        DevBuf<PropSeg> d_segs; DevBuf<PropRowRec> d_recs;
    } fwd, tr;
    bool t_built = false;
    DevBuf<int64_t> d_in_ptr, d_in_pos; DevBuf<int32_t> d_in_row; // [nc + 1], [edges], [edges]: the entries column by column
};
struct SubBufs {
    bool valid = false; uint64_t edges = 0;
    DevBuf<int64_t> d_ptr, d_eid, d_scan, d_base; DevBuf<int32_t> d_col;
    DevBuf<uint64_t> d_rtot, d_off; DevBuf<uint32_t> d_cnt; DevBuf<unsigned long long> d_tot;
    SubProp prop; bool prop_used = false; // (prop_used: prop holds something)
};

// The loose words of the context, grouped by role.
struct Params { // fora_hip_set_params / _raw
    bool have = false;
    double alpha = 0.2, epsilon = 0.5, rmax_scale = 1.0, rmax = 0, omega = 0;
    int opt = 0; uint64_t seed = 0;
};
struct Balanced { // --balanced (query.h:848-884): cost model in seconds (fora_hip_set_balanced), per-slot results of the last batch
    bool on = false;
    double c_pop = 2.0e-11, c_edge = 2.4e-11, t_walk = 6.5e-11, t_idx = 2.2e-11, start = 8;
    std::vector<double> h_rmax_used; std::vector<int32_t> h_rounds;
};
struct TeamState { // run state of the team push (fora_team.h)
    bool dirty = false;        // a launch ended with an error flag: its reserve accumulators (TeamDev::rsvl) may not be zero
    bool timeout_seen = false; // the last device error was ERR_TEAM_TIMEOUT (with_bucket_retry runs the call again without the team push)
    int suspend = 0;           // calls left that push with the bucketed kernels after a team time-out
    uint64_t fallbacks = 0;    // calls re-run that way so far (fora_hip_get_option "team_fallbacks")
    bool coop_ok = false;      // launch k_push_team cooperatively (option team_coop, device attribute)
    bool coop_failed = false;  // hipLaunchCooperativeKernel refused once: plain launches from then on
};
struct BucketRetry { // see with_bucket_retry
    uint32_t scale = 1;      // bucket capacity multiplier, doubled after a bucket overflow
    uint32_t scale_topk = 1; // ... of the calls that plan with a divisor (div > 1: the top-k driver on wide graphs).  Its own word: those calls start at 1 / 16 of a
                             // query's buckets and overflow far more often; a doubling there must not shrink the batches of later query / power-iteration calls
    uint32_t div = 1;        // bucket capacity divisor of the call in progress (top-k: TOPK_BK_DIV on wide graphs, plan_workspace).  Not part of
                             // the plan: a kept workspace may have been planned under another call's divisor
    bool overflow = false;   // the last device error was ERR_BUCKET_OVERFLOW
    uint64_t retries = 0;    // calls re-run with doubled buckets so far (fora_hip_get_option "bucket_retries")
};
struct Timing { // event pairs of the launches (EvSpan, ev_collect) and what they add up to
    bool profiling = true;
    std::vector<EvPair> ev_pool; size_t ev_used = 0;
    fora_timing total{};
    double bwd_ms = 0, combine_ms = 0, sp_compact_ms = 0, seed_combine_ms = 0, sw_compact_ms = 0, sw_sort_ms = 0, sw_cut_ms = 0, prop_gather_ms = 0, prop_combine_ms = 0, propt_transpose_ms = 0, tk_select_ms = 0, sddmm_ms = 0, softmax_ms = 0, attn_ms = 0, store_ms = 0, cols_ms = 0, sub_ms = 0, subp_t_ms = 0, subp_short_ms = 0, subp_long_ms = 0; // of the call in progress (EV_BWD, EV_COMBINE, EV_SP_COMPACT, EV_SEED_COMBINE)
};

struct fora_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipDeviceProp_t prop{};
    std::string err;
    Tunables opt_;
    int grid_blocks = 2048; // (option `grid`)
    Graph g; Index ix; Workspace ws; BwdBufs bw; SparseResult sp; SeedBufs sd; SweepResult swp; PropBufs pr; PropTBufs pt; RowStore st; ColsBufs cl; SubBufs sb;
    bool topk_lds_ready = false; // k_topk_rows<true> may take the whole of a CU's LDS (topk_lds_limit)
    uint64_t sparse_gen = 0;   // fora_hip_get_option "sparse_generation": counts the times a sparse result became held or stopped being held
    int batch_req = 0;        // the caller's request (fora_hip_set_batch), not part of a plan
    uint64_t bin_launches = 0; // parity picks the counter set
    std::vector<QState> h_qs;
    Params par; Balanced bal; TeamState team_run; BucketRetry retry; Timing tm;
    DevBuf<unsigned long long> d_stamps; // diagnostic builds (-DFORA_STAMPS)
};

namespace {

int fail(fora_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}

#define HIPCHK(c, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(c, e_ == hipErrorOutOfMemory ? FORA_E_NOMEM : FORA_E_HIP,               \
                        std::string(#call) + ": " + hipGetErrorString(e_));                      \
    } while (0)

// every buffer of the group freed, every field of it back at its initialiser
void free_graph(fora_ctx *c) { c->g = Graph{}; }
// what SUBGRAPH PRODUCTS derived from the held subgraph goes: the subgraph ends or is built again
void sub_prop_drop(fora_ctx *c) {
    if (!c->sb.prop_used) return;
    (void)hipSetDevice(c->device);
    c->sb.prop = SubProp{}; c->sb.prop_used = false;
}
// the held sparse result stops being held (its arrays stay): the generation moves, the transposition built from it goes
void sparse_unheld(fora_ctx *c) {
    if (c->sp.valid) c->sparse_gen++;
    c->sp.valid = false; c->sp.entries = 0;
    c->sp.compacted = false; c->sp.cols = 0;
    c->sb.valid = false; c->sb.edges = 0; // (the subgraph over its columns)
    sub_prop_drop(c);
    if (c->pt.built) { (void)hipSetDevice(c->device); c->pt = PropTBufs{}; }
}
void free_sparse(fora_ctx *c) { sparse_unheld(c); c->sp = SparseResult{}; }
void free_sweep(fora_ctx *c) { c->swp = SweepResult{}; }
void free_prop(fora_ctx *c) { c->pr = PropBufs{}; }
void free_store(fora_ctx *c) { c->st = RowStore{}; }
void free_cols(fora_ctx *c) { c->cl = ColsBufs{}; }
void free_sub(fora_ctx *c) { c->sb = SubBufs{}; }
// the columns of the held sparse result: the n nodes, or its own nc once fora_hip_sparse_compact has relabelled it.  Every call
// on the held rows sizes and plans its column side by this
inline uint64_t held_cols(const fora_ctx *c) { return c->sp.compacted ? c->sp.cols : (uint64_t)c->g.n; }
void free_index(fora_ctx *c) { c->ix = Index{}; }
void free_workspace(fora_ctx *c) { c->ws = Workspace{}; }

constexpr size_t N_COUNTERS = 2 * (size_t)(MAX_LEVELS + 2) + 2;
// workgroups per slot of the kernels that sweep a slot's slab (walk allocation, top-k frontier / copy / count): ~32 k
// workgroups per launch; one per 256 nodes (up to 1 M tiny workgroups at 1000 slots) cost k_walk_alloc 19 ms instead of
// 8 per 3000 ws queries
static uint32_t slab_grid_x(const fora_ctx *c, int nq) {
    const int64_t nchunk = ((int64_t)c->g.n + BLOCK - 1) / BLOCK;
    int64_t x = std::min<int64_t>(1024, std::max<int64_t>(16, 32768 / std::max(1, nq)));
    if (c->opt_.ax > 0) x = c->opt_.ax;
    return (uint32_t)std::max<int64_t>(1, std::min<int64_t>(std::min(x, nchunk), 65535)); // (may be a grid's y extent: Dev::slot_major)
}
static unsigned walk_grid_x(const fora_ctx *c, int nq) {
    if (c->opt_.wx > 0) return (unsigned)c->opt_.wx;
    // ~24 k workgroups per launch (1280 are resident): ws at 1000 slots, blocks per slot 4 -> 552 ms, 8 -> 509,
    // 16 -> 493, 24 -> 489, 32 -> 495 per 3000 queries
    return (unsigned)std::min(2048, std::max(16, 24576 / std::max(1, nq)));
}

constexpr int SPEC = 3;          // levels launched ahead of the frontier-size readback
constexpr int FLC_RING = SPEC + 2;

static bool want_binned(const fora_ctx *c) { return c->opt_.direct != 1; } // direct: the one-atomic-per-edge path (tests)
// bins handled per pass in the wide layout (graphs with more bins run several bin/accum passes per level)
static int want_pass_bins(const fora_ctx *c, int nbins) {
    // graphs with more than 1024 bins run several passes per level; up to 2560 bins per pass then (the per-pass
    // re-scan of the frontier and of the walk index costs more than the shorter message runs: Twitter-2010-sized,
    // 26 queries, bins per pass 256 / 512 / 1024: 7.5 / 4.3 / 3.0 s)
    const int cap = nbins > MAX_BINS_WIDE ? MAX_BINS_HUGE : MAX_BINS_WIDE;
    if (c->opt_.pass_bins > 0) return (int)std::min<int64_t>(c->opt_.pass_bins, cap);
    if (nbins > cap) { const int np = (nbins + cap - 1) / cap; return (nbins + np - 1) / np; } // equal passes
    return cap;
}
// narrow layout: <= MAX_BINS bins and the slice index fits the 4-byte push message
static bool want_wide(const fora_ctx *c) {
    if (c->opt_.force_wide == 1) return true; // tests: exercise the wide layout on small graphs
    return !((uint64_t)c->g.n <= (uint64_t)MAX_BINS * BIN_SIZE && (uint64_t)c->g.n <= (1ull << SEG_BITS));
}
// bits of a node id inside its bin: 8192-node bins in the narrow layout, 16384 in the wide ones
static int bin_shift(const fora_ctx *c) { return want_wide(c) ? BIN_SHIFT_WIDE : BIN_SHIFT; }
static uint64_t bins_of(const fora_ctx *c) { const int sh = bin_shift(c); return ((uint64_t)c->g.n + (1ull << sh) - 1) >> sh; }
static uint32_t want_bk_cap(const fora_ctx *c) {
    if (c->opt_.bkcap > 0) return (uint32_t)c->opt_.bkcap;
    return 163840; // walk results: ~omega*rsum/nbins per bucket (ws: ~110 k)
}
static uint32_t want_bk_cap_wide(const fora_ctx *c) { // messages per (slot, bin) bucket: push increments and indexed walk results (online ones go by direct atomics)
    if (c->opt_.bkcap > 0) return (uint32_t)c->opt_.bkcap;
    // a dense level relaxes about every edge once: nnz / nbins messages per bin on average (Twitter-2010-sized: 289 k),
    // hubs' bins beyond that use the overflow list; 196608 covers the indexed walk results (~omega*rsum/nbins per bucket)
    const uint64_t nbins = bins_of(c);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(196608, (uint64_t)(1.4 * (double)c->g.nnz / (double)std::max<uint64_t>(1, nbins))), 1u << 26);
}

// (the wide / narrow choice changes bk_cap, which forces a re-plan of the workspace)
// sub-buckets per (slot, bin) = producer workgroups per slot (Dev::bk_w): ~16 k producer workgroups per launch
static uint32_t want_sub(const fora_ctx *c, int slots) {
    if (c->opt_.xb > 0) return (uint32_t)std::min<int64_t>(c->opt_.xb, MAX_SUB);
    // wide: 512-thread producers, 2-3 resident per CU.  LJ-sized, 74 slots: 16 -> 549 ms per 148 queries, 32 -> 492, 64 -> 515,
    // 128 -> 539; Twitter-sized, 12 slots, 24 queries: 32 -> 2438 ms, 64 -> 2010, 128 -> 1576 (few slots: the tiles of a level
    // have to be dealt to many workgroups)
    // (16384-node bins, LJ-sized, 140 slots, 280 queries: 16 -> 902 ms, 32 -> 840, 64 -> 826)
    if (want_wide(c)) return slots >= 256 ? 32u : slots >= 32 ? 64u : (uint32_t)MAX_SUB;
    return (uint32_t)std::min(MAX_SUB, std::max(16, 16384 / std::max(1, slots)));
}
// the whole plan of a workspace of `slots` slots (but team_rlog_cap, see WsPlan); reads the graph, the options and BucketRetry only
static WsPlan plan_workspace(const fora_ctx *c, double omega_hint, int slots) {
    WsPlan p;
    const uint64_t n = (uint64_t)c->g.n;
    p.binned = want_binned(c);
    p.segs = n + (uint64_t)c->g.nnz / PUSH_SEG + 64;
    double walks = omega_hint > 0 ? omega_hint : 0;
    if (walks > 4e12) walks = 4e12;
    p.wit_cap = n + n / WALK_SEG + (uint64_t)(walks / WALK_SEG) + 64;
    if (p.binned) {
        p.nbins = (int)bins_of(c);
        p.pbins = want_wide(c) ? std::min(p.nbins, want_pass_bins(c, p.nbins)) : std::max(p.nbins, (int)c->g.walk.dg.nbx); // narrow: the walk results in bucket order may need a bin more
        p.sub = want_sub(c, slots);
        { // capacity of one sub-bucket: the bucket's capacity over its sub-buckets (+25 % for uneven producers); the
          // `bkcap` option (tests) sets it directly
            const uint64_t total = (uint64_t)(want_wide(c) ? want_bk_cap_wide(c) : want_bk_cap(c));
            uint64_t cap = c->opt_.bkcap > 0 ? total : (total + total / 4 + p.sub - 1) / p.sub;
            // the top-k driver's rounds push from small frontiers (delta starts at 1 / 10k): its buckets start at 1 / BucketRetry::div of
            // a query's -- a slot is a fifth of the memory, a batch holds that many more of them, and every per-round launch
            // (k_push_tail: ONE workgroup per slot; the slab sweeps; the walk kernels) works on that many more slots at once.
            // A round that does overflow is run again with doubled buckets like any other (with_bucket_retry)
            cap = std::min<uint64_t>(std::max<uint64_t>(cap * (c->retry.div > 1 ? c->retry.scale_topk : c->retry.scale) / std::max<uint32_t>(1, c->retry.div), 64), 1u << 28);
            // whole 128-byte lines: every sub-bucket then starts on one, which the aligned flush of k_walk_dg counts on
            p.bk_cap = (uint32_t)((cap + FLUSH_LINE_MAX - 1) & ~(uint64_t)(FLUSH_LINE_MAX - 1));
            assert(p.bk_cap % FLUSH_LINE_MAX == 0 && FLUSH_LINE_MAX * sizeof(uint64_t) == 128);
        }
        p.segq_cap = n;
        p.ov_cap = c->opt_.ovcap > 0 ? (uint32_t)c->opt_.ovcap : (uint32_t)std::max<uint64_t>(262144, n / 8); // scales with the graph; the option: tests
        p.dbm_words = (uint32_t)((uint64_t)p.nbins << (bin_shift(c) - 6));
        p.scratch = (p.wit_cap * sizeof(WalkItemP) + 95) / 96 * 96; // whole PushSeg (24 B) and WalkItemP (32 B) entries
        p.per_slot = n * 8 * 2 + n * 4 * 2 + p.segq_cap * 8 * 2 + std::max<uint64_t>(262144, n / 8) * 12 + (uint64_t)p.pbins * p.sub * p.bk_cap * (want_wide(c) ? 8 : 12) + p.scratch +
                     (c->opt_.defer > 0 ? n * 4 * 2 : 0) + n / 4 + 64 + (uint64_t)p.sub * c->g.hub.hubs * 8; // + deferred lists and bitmaps, hub sums
    } else {
        p.scratch = (std::max(p.segs * sizeof(PushSeg), p.wit_cap * sizeof(WalkItemP)) + 95) / 96 * 96;
        p.per_slot = n * 8 * 4 + p.scratch;
    }
    p.wl_cap = (uint64_t)slots * n;
    p.seg_cap = (uint64_t)slots * p.scratch / sizeof(PushSeg);
    return p;
}

// col as uploaded, back on the host (one element at least).  The graph keeps no host copy: 5.9 GB at Twitter-2010 size
int download_col(fora_ctx *c, std::vector<int32_t> &col) {
    col.resize((size_t)std::max<int64_t>(1, c->g.nnz));
    HIPCHK(c, hipMemcpy(col.data(), c->g.d_col.get(), (size_t)c->g.nnz * 4, hipMemcpyDeviceToHost));
    return FORA_OK;
}

// The derived forms of the graph.  Each function below decides whether this graph, with these options on this device, gets
// the form; fora_tables.h computes it; the vectors are uploaded into a local value that is moved in after the last step.

// Multi-pass graphs (more bins than one pass holds): row-sorted copy of col + per-row split offsets, so that every
// pass of k_pushq_bin reads only its own part of each popped row.  Built once per (graph, pass size).
int ensure_row_split(fora_ctx *c, int nbins, int pbins) {
    const int npass = pbins > 0 ? (nbins + pbins - 1) / pbins : 1;
    if (npass <= 1 || c->opt_.no_split) { c->g.split = RowSplit{}; return FORA_OK; }
    if (c->g.split.d_row_split && c->g.split.pbins == pbins) return FORA_OK;
    c->g.split = RowSplit{};
    std::vector<int32_t> col;
    if (int rd = download_col(c, col)) return rd;
    const SplitTables t = make_row_split(c->g.n, c->g.h_row_ptr.data(), std::move(col), npass, pbins, bin_shift(c));
    RowSplit rs;
    if (!t.col_sorted.empty()) HIPCHK(c, rs.d_col_push.upload(t.col_sorted));
    HIPCHK(c, rs.d_row_split.upload(t.split));
    rs.pbins = pbins;
    c->g.split = std::move(rs);
    return FORA_OK;
}

// Team push (fora_team.h): members per team for this graph (0: the graph does not take the team path), the copy of
// col that names every target as (owner, local id) and the exact bucket capacities.  Built on first use and whenever
// the `team` / `team_size` options ask for another shape.
static bool want_team(const fora_ctx *c) {
    const bool on = c->opt_.team != 0; // (round 6: also for graphs with many dangling nodes -- 29.7 against 41.7 ms on the R-MAT ws variant, profiles/r06_dangling_team.txt)
    return on && want_binned(c) && !want_wide(c) && c->g.nnz > 0 && c->g.nnz < (1ll << 32); // (rowl / colt / off index edges with 32 bits)
}
int ensure_team(fora_ctx *c) {
    const bool want = want_team(c);
    const uint32_t force = (uint32_t)std::min<int64_t>(std::max<int64_t>(c->opt_.team_size, 0), TEAM_MAX);
    const uint32_t hubs_opt = (uint32_t)std::min<int64_t>(std::max<int64_t>(c->opt_.team_hubs, 0), 4096);
    if (c->g.team.checked && want == c->g.team.wanted && (!want || (c->g.team.force == force && c->g.team.hubs_opt == hubs_opt))) return FORA_OK;
    c->g.team = TeamTables{};
    TeamTables tb;
    tb.checked = true; tb.wanted = want; tb.force = force; tb.hubs_opt = hubs_opt;
    const auto done = [&] { c->g.team = std::move(tb); return FORA_OK; }; // (with T == 0: looked at, not taken -- a complete state too)
    if (!want) return done();
    std::vector<int32_t> col;
    if (int rd = download_col(c, col)) return rd;
    const uint32_t max_members = (uint32_t)std::min(TEAM_MAX, std::max(1, c->prop.multiProcessorCount * TEAM_WGS_PER_CU));
    const TeamLayout t = make_team_layout(c->g.n, c->g.h_row_ptr.data(), col.data(), force, max_members, hubs_opt);
    if (!t.T) return done();
    HIPCHK(c, tb.d_colt.upload(t.colt, t.colt.size() + 4)); // (a lane without a quad of its own loads quad 0: there is one)
    HIPCHK(c, tb.d_rowq.upload(t.rowq.data(), (size_t)c->g.n));
    HIPCHK(c, tb.d_off.upload(t.off));
    HIPCHK(c, tb.d_n2l.upload(t.n2l));
    HIPCHK(c, tb.d_l2n.upload(t.l2n));
    HIPCHK(c, tb.d_deg16.upload(t.deg16));
    HIPCHK(c, tb.d_hubtgt.upload(t.hubtgt));
    HIPCHK(c, tb.d_rowl.upload(t.rowl));
    tb.H = t.H; tb.T = t.T; tb.R = t.R; tb.cap = t.cap;
    return done();
}

// Hub pre-aggregation of the narrow push (Dev::col_hub): the `hubs` nodes of largest in-degree (ties: lower id), numbered in
// id order so that the hubs of a bin are a contiguous range, and a copy of col that names them by that number.
int build_hub_copy(fora_ctx *c, const int32_t *col) {
    c->g.hub = HubCopy{}; // (a rebuild: ensure_workspace)
    const int64_t nnz = c->g.nnz;
    const int64_t wide_auto = nnz <= (1ll << 28) ? 2048 : 0;
    // the hub sums live in the bin kernel's dynamic LDS next to its static arrays: 48 KB in the narrow and the 512-thread
    // wide kernel, 32 KB in the 1024-thread one (its stage of 12 edges per thread takes 122 of the 160 KB)
    const uint64_t nbins_all = bins_of(c);
    const int64_t lds_cap = !want_wide(c) ? 6144 : nbins_all > (uint64_t)MAX_BINS_WIDE ? 4096 : 6144;
    // 4096 only when this graph really takes the team path (ensure_team has built its tables: then the bin kernel never runs
    // and k_push_tail is the copy's only reader); a graph the team path rejects pushes with the bin kernel, which wants 1024
    const bool for_team = want_team(c) && c->g.team.T != 0;
    c->g.hub.for_team = for_team; // (no copy, for this path: a complete state too -- also after a failure below: ensure_workspace does not try again, the graph pushes without hub sums until the next set_graph, as before)
    const int64_t narrow_auto = for_team ? 4096 : 1024;
    const int64_t want = std::min<int64_t>(std::max<int64_t>(want_wide(c) ? (c->opt_.hubs_wide < 0 ? wide_auto : c->opt_.hubs_wide) : (c->opt_.hubs < 0 ? narrow_auto : c->opt_.hubs), 0), lds_cap);
    if (want == 0 || nnz == 0 || c->opt_.direct == 1) return FORA_OK;
    if (want_wide(c) && (int64_t)nbins_all > (int64_t)want_pass_bins(c, (int)nbins_all)) return FORA_OK; // several bin passes per level: the passes read the row-sorted copy, hubs are never used (make_dev)
    const HubTables t = make_hub_tables(c->g.n, col, (size_t)nnz, (size_t)want, bin_shift(c));
    HubCopy hc;
    HIPCHK(c, hc.d_col_hub.upload(t.col_hub));
    HIPCHK(c, hc.d_hub_node.upload(t.hub_node));
    HIPCHK(c, hc.d_hub_first.upload(t.hub_first));
    hc.hubs = (uint32_t)t.hub_node.size();
    hc.shift = bin_shift(c);
    hc.for_team = for_team;
    c->g.hub = std::move(hc);
    return FORA_OK;
}

// Quad-padded copies of col (and of the hub copy) for the wide bin kernel (Dev::col4), built on the device from what
// set_graph has uploaded; only for graphs that run the wide layout in one bin pass per level.
int build_quad_copies(fora_ctx *c) {
    c->g.quad = QuadCopies{};
    if (!want_binned(c) || !want_wide(c) || c->g.nnz == 0 || c->opt_.quads == 0) return FORA_OK;
    const uint64_t nbins_all = bins_of(c);
    if ((int64_t)nbins_all > (int64_t)want_pass_bins(c, (int)nbins_all)) return FORA_OK; // several passes per level: pass-split rows, edge by edge
    const size_t n = (size_t)c->g.n;
    // (Round 6, measured and dropped: rows placed so that each touches as few 64-byte lines as its length allows -- a row that would
    // straddle one line more than ceil(quads / 4) started at the next line.  LJ-sized bin kernel 315.4 / 314.8 ms against 320.7 / 314.5
    // back to back, Twitter-2010-sized 593.6 / 592.9 against 594.5 / 585.6: what a quad load costs is not the lines its row touches.)
    const QuadRows t = make_quad_rows(c->g.n, c->g.h_row_ptr.data());
    if (t.quads >= (1ull << 40)) return FORA_OK;
    // The copies are an optimisation (make_dev falls back to single-edge reads without them): they must never make
    // set_graph fail.  Not built when they would take more than a quarter of the free memory (the slots need it more);
    // an allocation that fails all the same leaves "no quads", not an error.
    const uint64_t qbytes = std::max<uint64_t>(1, t.quads) * 16, need = n * 8 + qbytes * (c->g.hub.d_col_hub ? 2 : 1);
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    if (need > fr / 4) return FORA_OK;
    QuadCopies qc;
    auto give_up = [&]() { (void)hipGetLastError(); return FORA_OK; };
    if (qc.d_rowinfo4.upload(t.rowinfo4) != hipSuccess) return give_up();
    if (qc.d_col4.alloc(qbytes / 4) != hipSuccess) return give_up();
    const unsigned grid = (unsigned)std::min<size_t>((n + BLOCK - 1) / BLOCK, 1u << 20);
    hipLaunchKernelGGL(k_pad_quads, dim3(grid), dim3(BLOCK), 0, c->stream, c->g.n, (const int64_t *)c->g.d_row_ptr.get(), (const int32_t *)c->g.d_col.get(),
                       (const uint64_t *)qc.d_rowinfo4.get(), qc.d_col4.get());
    if (c->g.hub.d_col_hub) {
        if (qc.d_col_hub4.alloc(qbytes / 4) != hipSuccess) return give_up();
        hipLaunchKernelGGL(k_pad_quads, dim3(grid), dim3(BLOCK), 0, c->stream, c->g.n, (const int64_t *)c->g.d_row_ptr.get(), (const int32_t *)c->g.hub.d_col_hub.get(),
                           (const uint64_t *)qc.d_rowinfo4.get(), qc.d_col_hub4.get());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    qc.quads = t.quads;
    c->g.quad = std::move(qc);
    return FORA_OK;
}

// Degree-grouped walk copy (WalkDG, fora_kernels.h) of graphs that run the narrow layout: H hub records + at most 255
// out-degree classes whose tables fit a workgroup's LDS share.  Graphs that do not qualify keep k_walk_online.
int build_walk_dg(fora_ctx *c, const int64_t *row_ptr, const int32_t *col) {
    c->g.walk = WalkCopy{};
    const int32_t n = c->g.n;
    const int64_t nnz = c->g.nnz;
    if (c->opt_.walk_dg == 0 || c->opt_.no_compact == 1 || nnz >= (1ll << 31) || nnz == 0) return FORA_OK;
    if (!((uint64_t)n <= (uint64_t)MAX_BINS * BIN_SIZE && (uint64_t)n <= (1ull << SEG_BITS))) return FORA_OK; // narrow layout only
    const DgTables t = make_walk_dg(n, row_ptr, col, c->opt_.dg_hubs);
    if (!t.have) return FORA_OK;
    WalkCopy wc;
    HIPCHK(c, wc.d_perm.upload(t.perm));
    HIPCHK(c, wc.d_inv.upload(t.inv));
    HIPCHK(c, wc.d_colp.upload(t.colp));
    HIPCHK(c, wc.d_rec.upload(t.rec, 1));
    HIPCHK(c, wc.d_T.upload(t.T));
    if (t.nbx) HIPCHK(c, wc.d_invb.upload(t.invb));
    WalkDG g{};
    g.invb = wc.d_invb.get(); g.nbx = t.nbx; g.nbx_magic = t.nbx_magic;
    g.perm = wc.d_perm.get(); g.inv = wc.d_inv.get(); g.colp = wc.d_colp.get(); g.rec = wc.d_rec.get(); g.T = wc.d_T.get();
    g.H = t.H; g.nrec = t.nrec; g.nblk = (uint32_t)t.T.size(); g.ts = t.ts; g.bits = t.bits; g.zero_first = t.zero_first;
    g.bits32 = t.bits32;
    wc.dg = g;
    c->g.walk = std::move(wc);
    return FORA_OK;
}

// Team push: bytes per team of its workspace buffers with reserve logs of `logcap` entries -- message buffers + increment
// tables (two parities), rsvl, reserve logs, words
static uint64_t team_bytes_per_team(const fora_ctx *c, uint64_t logcap) {
    const uint64_t T = c->g.team.T;
    return 2 * c->g.team.cap * 4 + 3 * T * (c->g.team.R + 64 + c->g.team.H) * 8 + T * logcap * 10 + 2 * T * T * 8;
}
// Words of Workspace::d_team_ctl: [0] next slot, [32] abort | from `sync`: the sync words | from `slot_seq`: the slot sequences
struct TeamCtl { size_t sync, slot_seq, total; };
static TeamCtl team_ctl_layout(uint32_t nteams, int slots) {
    const size_t sync = 64, slot_seq = sync + (size_t)nteams * 5 * 16 * 2;
    return {sync, slot_seq, slot_seq + (size_t)nteams * ((size_t)slots + 2)};
}
int team_fits(fora_ctx *c, Workspace &w);
int ensure_workspace(fora_ctx *c, int want_slots, double omega_hint) {
    if (!c->g.n) return fail(c, FORA_E_ARG, "set_graph first");
    if (int rt = ensure_team(c)) return rt;
    if (c->opt_.hubs < 0 && !want_wide(c) && c->g.hub.for_team != (want_team(c) && c->g.team.T != 0)) {
        // the `team` / `team_size` options changed which push this graph takes: the hub copy follows (see build_hub_copy)
        std::vector<int32_t> col;
        if (int rd = download_col(c, col)) return rd;
        free_workspace(c);
        if (int rh = build_hub_copy(c, col.data())) return rh;
        if (int rq = build_quad_copies(c)) return rq;
    }
    {
        // An existing workspace is kept if it has enough slots -- as many as the call can use (its queries, at most 1024, at most what memory allowed when
        // the workspace was planned) --, team buffers exactly when the graph takes the team path, and a plan that fits the one this call would make for its slots.
        int need = c->batch_req > 0 ? c->batch_req : std::min(want_slots > 0 ? want_slots : 1024, 1024);
        if (c->batch_req == 0 && c->ws.B > 0 && c->ws.B_memcap > 0) need = std::min(need, c->ws.B_memcap);
        if (c->ws.B > 0 && c->ws.B >= need && (c->g.team.T != 0) == bool(c->ws.d_team_msg)) {
            const WsPlan pe = plan_workspace(c, omega_hint, c->ws.B);
            if (c->ws.plan.fits(pe)) return ensure_row_split(c, pe.nbins, pe.pbins);
        }
    }
    int B = c->batch_req > 0 ? c->batch_req : 0;
    if (B == 0) {
        // the slot count follows from the FREE memory: give the old workspace back first, or a re-plan (larger walk budget
        // of a top-k call, other sub-bucket count, more queries) would size itself from what the old one left over
        free_workspace(c);
        size_t fr = 0, tot = 0;
        HIPCHK(c, hipMemGetInfo(&fr, &tot));
        uint64_t budget = (uint64_t)(fr * 0.75);
        if (c->g.team.T) { // the team push's own buffers (allocated below) come out of the same memory
            const uint64_t T = c->g.team.T, nt = std::max<uint64_t>(1, (uint64_t)c->prop.multiProcessorCount * TEAM_WGS_PER_CU / T);
            const uint64_t team_bytes = nt * team_bytes_per_team(c, 1u << 17);
            budget -= std::min<uint64_t>(budget / 2, team_bytes);
        }
        const uint64_t per_slot = plan_workspace(c, omega_hint, 1024).per_slot; // bytes per slot hardly depend on the slot count (sub-bucket rounding)
        B = (int)std::min<uint64_t>(1024, std::max<uint64_t>(1, budget / per_slot)); // ws, 1000 queries: 2845 q/s at 256, 3035 at 512, 3101 at 1000
    }
    B = std::max(1, B);
    const int memcap = B;
    if (want_slots > 0 && c->batch_req == 0) B = std::min(B, std::max(want_slots, 1));
    free_workspace(c);
    Workspace w; // moved into c->ws after the last step: a failure on the way leaves no workspace
    w.plan = plan_workspace(c, omega_hint, B);
    WsPlan &p = w.plan;
    const uint64_t slab = p.wl_cap;
    const size_t ctr = (size_t)B * CSTRIDE; // one counter line per slot
    HIPCHK(c, w.d_residue.alloc(slab));
    HIPCHK(c, w.d_ppr.alloc(slab));
    if (p.binned) {
        for (auto &fl : w.d_fl) HIPCHK(c, fl.alloc(slab));
        HIPCHK(c, w.d_fl_count.alloc(2 * ctr));
        for (auto &tab : w.d_inc_tab) HIPCHK(c, tab.alloc((uint64_t)B * p.segq_cap));
        HIPCHK(c, w.d_ov_w.alloc((uint64_t)B * p.ov_cap));
        HIPCHK(c, w.d_ov_inc.alloc((uint64_t)B * p.ov_cap));
        HIPCHK(c, w.d_ov_count.alloc(2 * ctr));
        HIPCHK(c, w.d_ov_bin.alloc(2 * (size_t)B * p.nbins));
        const uint64_t buckets = (uint64_t)B * p.pbins * p.sub;
        if (!want_wide(c)) HIPCHK(c, w.d_bk_w.alloc(buckets * p.bk_cap)); // wide: one 64-bit word per message in bk_inc
        HIPCHK(c, w.d_bk_inc.alloc(buckets * p.bk_cap));
        HIPCHK(c, w.d_bk_count.alloc(buckets));
        HIPCHK(c, w.h_flc.alloc((size_t)FLC_RING * ctr));
        HIPCHK(c, w.d_dbm.alloc(2 * (size_t)B * p.dbm_words));
        HIPCHK(c, w.d_dflag.alloc(2 * (size_t)B * p.nbins));
        if (c->opt_.defer > 0) HIPCHK(c, w.d_dl.alloc(2 * slab)); // k_push_tail's deferred lists: only with the option (changing it re-plans the workspace)
        if (c->g.hub.hubs && c->g.hub.shift == bin_shift(c)) HIPCHK(c, w.d_hubsum.alloc((size_t)B * p.sub * c->g.hub.hubs));
        if (c->g.team.T) { // team push: message buffers of every team (two parities), bucket counts, control words
            const uint32_t T = c->g.team.T;
            uint32_t nteams = std::max<uint32_t>(1, (uint32_t)c->prop.multiProcessorCount * TEAM_WGS_PER_CU / T);
            if (c->opt_.team_max > 0) nteams = std::min<uint32_t>(nteams, (uint32_t)c->opt_.team_max);
            size_t fr = 0, tot = 0;
            HIPCHK(c, hipMemGetInfo(&fr, &tot));
            // pops of one member in one slot (ws-sized graph at eps 0.5: 43 k on average); beyond it: rsvl.  Tight memory: shorter logs
            p.team_rlog_cap = 1u << 17;
            while (p.team_rlog_cap > 1024 && team_bytes_per_team(c, p.team_rlog_cap) > fr / 4) p.team_rlog_cap /= 2;
            nteams = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nteams, (uint64_t)(fr / 2) / std::max<uint64_t>(1, team_bytes_per_team(c, p.team_rlog_cap))));
            const size_t members = (size_t)nteams * T;
            HIPCHK(c, w.d_team_msg.alloc((size_t)nteams * 2 * c->g.team.cap + 16 + diag::TEAM_MSG_PROBE_WORDS)); // (probe words: 0 in the product build)
            HIPCHK(c, w.d_team_inct.alloc(members * 2 * (c->g.team.R + 64 + c->g.team.H)));
            HIPCHK(c, w.d_team_rsvl.alloc(members * c->g.team.R));
            HIPCHK(c, w.d_team_rsvl.zero(c->stream)); // every slot leaves it zero again
            HIPCHK(c, w.d_team_rlog_id.alloc(members * p.team_rlog_cap));
            HIPCHK(c, w.d_team_rlog_val.alloc(members * p.team_rlog_cap));
            HIPCHK(c, w.d_team_cnt.alloc(members * 2 * T));
            HIPCHK(c, w.d_team_ctl.alloc(team_ctl_layout(nteams, B).total));
            w.team_n = nteams;
            if (int rf = team_fits(c, w)) return rf;
        }
    } else {
        for (auto &wl : w.d_wl) HIPCHK(c, wl.alloc(slab));
    }
    HIPCHK(c, w.d_scratch.alloc((uint64_t)B * p.scratch));
    HIPCHK(c, w.d_wit_count.alloc(ctr));
    HIPCHK(c, w.d_sw.alloc(2 * ctr));
    HIPCHK(c, w.d_sw.zero(c->stream)); // self-resetting
    HIPCHK(c, w.d_tile_ctr.alloc(2 * ctr));
    HIPCHK(c, w.d_tile_ctr.zero(c->stream)); // every launch zeroes the set of the next one
    HIPCHK(c, w.d_counters.alloc(N_COUNTERS));
    HIPCHK(c, w.d_qs.alloc((size_t)B));
    HIPCHK(c, w.d_src.alloc((size_t)B));
    HIPCHK(c, w.d_err.alloc(1));
    HIPCHK(c, w.h_pinned.alloc(MAX_LEVELS + 2));
    HIPCHK(c, w.h_qs_pin.alloc((size_t)B));
    HIPCHK(c, w.h_steps_pin.alloc(1));
    w.B = B; w.B_memcap = memcap;
    if (int rs = ensure_row_split(c, p.nbins, p.pbins)) return rs;
    c->ws = std::move(w);
    c->h_qs.resize(B);
    return FORA_OK;
}

Dev make_dev(fora_ctx *c, int nq, bool with_idx, double rmax = -1, double omega = -1) {
    if (rmax < 0) rmax = c->par.rmax;
    if (omega < 0) omega = c->par.omega;
    Dev d{};
    const Workspace &w = c->ws;
    const WsPlan &p = c->ws.plan;
    const size_t B = (size_t)w.B, ctr = B * CSTRIDE;
    d.n = c->g.n; d.nq = nq;
    d.rowinfo = c->g.d_rowinfo.get(); d.row_ptr = c->g.d_row_ptr.get(); d.col = c->g.d_col.get(); d.deg = c->g.d_deg.get();
    d.rp32 = c->g.d_rp32.get(); d.colp = c->g.d_colp.get(); d.colbits = c->g.colbits;
    d.colp32 = (uint64_t)c->g.nnz * c->g.colbits < (1ull << 32) ? 1 : 0;
    d.dg = c->g.walk.dg;
    d.residue = w.d_residue.get(); d.ppr = w.d_ppr.get(); d.wl_cap = p.wl_cap;
    d.seg = (PushSeg *)w.d_scratch.get(); d.seg_cap = p.seg_cap;
    d.wit = (WalkItemP *)w.d_scratch.get(); d.wit_cap = p.wit_cap;
    d.wl_count = w.d_counters.get();
    d.seg_count = w.d_counters.get() + (MAX_LEVELS + 2);
    d.wit_count = w.d_wit_count.get();
    d.tot_steps = w.d_counters.get() + 2 * (size_t)(MAX_LEVELS + 2) + 1;
    d.qs = w.d_qs.get(); d.src = w.d_src.get(); d.err = w.d_err.get();
    d.afix = (uint64_t)std::ldexp(c->par.alpha, 62);
    double t = std::ceil(std::ldexp(rmax, 62));
    d.t1 = t >= 9223372036854775808.0 ? (~0ull >> 1) : (t < 1.0 ? 1 : (uint64_t)t);
    d.alpha32 = (uint32_t)(c->par.alpha * 4294967296.0);
    d.seed_lo = (uint32_t)c->par.seed; d.seed_hi = (uint32_t)(c->par.seed >> 32);
    d.alpha = c->par.alpha; d.omega = omega; d.opt = c->par.opt;
    d.binned = p.binned ? 1 : 0; d.nbins = p.nbins; d.wide = p.binned && want_wide(c) ? 1 : 0;
    d.pbins = p.pbins; d.bin_lo = 0; d.bin_cnt = std::min(p.pbins, p.nbins);
    d.col_push = c->g.split.d_col_push.get() ? c->g.split.d_col_push.get() : c->g.d_col.get();
    d.row_split = c->g.split.d_row_split.get();
    d.npass = p.pbins > 0 ? (p.nbins + p.pbins - 1) / p.pbins : 1;
    d.pass = 0;
    d.acc_group = 1; // (set per launch: acc_grid)
    // Dispatch order of the wide kernels (Dev::slot_major), measured per kernel (profiles/r06_slot_major.txt): slot-major pays for the bin kernel
    // when a launch holds many slots (LJ-sized, 143 slots: 1135-1205 -> 1073-1107 ms per 1000 queries in A/B runs; Twitter-2010-sized, 8 slots:
    // 620 -> 930 ms) and for the indexed walks of query calls (LJ-sized ~ - 5 %, Twitter-2010-sized - 2 %); it loses for the accumulate, the walk
    // allocation and everything in the top-k drivers.  FETCH_SIZE and TCC hits / misses are the same in both orders: if it is reuse, it is in the memory-side Infinity Cache.
    d.slot_major = c->opt_.slot_major >= 0 ? (uint32_t)c->opt_.slot_major & 15u
                   : (c->retry.div > 1 ? 0u : (4u | (nq >= 32 ? 1u : 0u)));
    d.tiny_max = (uint32_t)std::min<int64_t>(std::max<int64_t>(c->opt_.tiny, 0), 1023); // 512: ws accum 116 -> 113 ms per 3000 queries against 128; 2048: 119, 8192: 193 (the crossing list of the small-bucket path holds 1024)
    for (int par = 0; par < 2; par++) { // the two parity sets of a pair are the halves of one buffer (null while it is empty)
        d.fl[par] = w.d_fl[par].get(); d.inc_tab[par] = w.d_inc_tab[par].get();
        d.fl_count[par] = w.d_fl_count.part(par, ctr); d.tile_ctr[par] = w.d_tile_ctr.part(par, ctr);
        d.ov_count[par] = w.d_ov_count.part(par, ctr); d.ov_bin[par] = w.d_ov_bin.part(par, B * p.nbins);
        d.dbm[par] = w.d_dbm.part(par, B * p.dbm_words); d.dflag[par] = w.d_dflag.part(par, B * p.nbins);
        d.dl[par] = w.d_dl.part(par, B * c->g.n); d.wl[par] = w.d_wl[par].get();
    }
    d.sw_count = w.d_sw.part(0, ctr); d.sw_done = w.d_sw.part(1, ctr);
    d.pop_next = 1;
    d.stamps = c->d_stamps.get();
    d.round_div = 0;
    d.rounds = 1; // the query / push entry points raise it (k_round_sweep); top-k, --balanced and power iteration drive their own rounds
    if (p.binned && c->g.hub.d_col_hub && w.d_hubsum && c->g.hub.shift == bin_shift(c) && p.pbins >= p.nbins) { // one pass per level only: the passes of larger graphs read a row-sorted copy
        d.col_hub = c->g.hub.d_col_hub.get(); d.hub_node = c->g.hub.d_hub_node.get(); d.hub_first = c->g.hub.d_hub_first.get(); d.hubsum = w.d_hubsum.get(); d.hubs = c->g.hub.hubs;
        d.hub_min = (uint32_t)std::min<int64_t>(std::max<int64_t>(c->opt_.hub_min, 1), 0x7FFFFFFF);
        d.tail_hubs = c->opt_.tail_hubs != 0 && (size_t)c->g.hub.hubs * 8 <= 40960 ? 1u : 0u; // (k_push_tail: 20 KiB of static LDS + the sums within 64 KiB)
    }
    if (d.wide && c->g.quad.d_col4 && !c->g.split.d_row_split && !c->g.split.d_col_push && c->opt_.quads != 0) { // one bin pass per level: the bin kernel reads quads
        d.col4 = c->g.quad.d_col4.get(); d.rowinfo4 = c->g.quad.d_rowinfo4.get();
        d.col_hub4 = d.col_hub ? c->g.quad.d_col_hub4.get() : nullptr;
        if (d.col_hub && !d.col_hub4) d.col4 = nullptr; // (no padded hub copy: edges one by one)
    }
    d.defer_k = TEST_PATHS && p.binned && w.d_dl ? (int32_t)std::min<int64_t>(std::max<int64_t>(c->opt_.defer, 0), 8) : 0; // the direct path keeps plain levels
    d.defer_min = (uint32_t)std::min<int64_t>(std::max<int64_t>(c->opt_.defer_min, 0), 0x7FFFFFFF);
    d.dbm_words = p.dbm_words; d.segq_cap = p.segq_cap;
    d.ov_w = w.d_ov_w.get(); d.ov_inc = w.d_ov_inc.get(); d.ov_cap = p.ov_cap;
    d.bk_w = w.d_bk_w.get(); d.bk_inc = w.d_bk_inc.get(); d.bk_count = w.d_bk_count.get(); d.bk_cap = p.bk_cap; d.sub = p.sub;
    d.flush_keep = (uint32_t)std::min<int64_t>(std::max<int64_t>(c->opt_.walk_flush_keep, 0), DG_STAGE);
    if (with_idx) { d.rw_idx = c->ix.d_rw_idx.get(); d.idx_off = c->ix.d_idx_off.get(); d.idx_cnt = c->ix.d_idx_cnt.get(); }
    return d;
}

// ---- event-pair timing of individual launches on the ctx stream
// One pair of the pool around a span of launches: begun by the constructor (or begin()), ended by end() where stream work follows that must
// stay outside the span, by the destructor otherwise -- so no return path leaves a pair open.  `profile` option off (or no event to be had): nothing.
class EvSpan {
    fora_ctx *c;
    int h = -1; // the pair in Timing::ev_pool; -1: none open
public:
    explicit EvSpan(fora_ctx *ctx) : c(ctx) {} // not begun yet
    EvSpan(fora_ctx *ctx, EvKind kind) : c(ctx) { begin(kind); }
    EvSpan(const EvSpan &) = delete; EvSpan &operator=(const EvSpan &) = delete;
    ~EvSpan() { end(); }
    void begin(EvKind kind) {
        end();
        Timing &t = c->tm;
        if (!t.profiling) return;
        if (t.ev_used == t.ev_pool.size()) {
            EvPair p{};
            if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return;
            t.ev_pool.push_back(p);
        }
        EvPair &p = t.ev_pool[t.ev_used];
        p.kind = kind;
        (void)hipEventRecord(p.a, c->stream);
        h = (int)t.ev_used++;
    }
    void end() { if (h >= 0) (void)hipEventRecord(c->tm.ev_pool[h].b, c->stream); h = -1; }
};
void ev_collect(fora_ctx *c) { // call after the stream is idle
    Timing &t = c->tm;
    for (size_t i = 0; i < t.ev_used; i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, t.ev_pool[i].a, t.ev_pool[i].b) != hipSuccess) continue;
        fora_timing &f = t.total;
        switch (t.ev_pool[i].kind) {
        case EV_PUSH_POP: f.push_pop_ms += ms; f.push_pop_launches++; break;          // k_push_pop (direct path)
        case EV_PUSH_EXPAND: f.push_expand_ms += ms; f.push_expand_launches++; break; // k_push_expand; the bin kernels k_pushq_bin
        case EV_WALK_ALLOC: f.walk_alloc_ms += ms; break;                             // k_walk_alloc
        case EV_WALK: f.walk_ms += ms; f.walk_launches++; break;                      // k_walk_idx (wide: with its accumulate passes), k_walk_dg / k_walk_online, k_walk_mc
        case EV_OTHER: f.other_ms += ms; break;                                       // resets, k_init_batch, k_topk_frontier, k_copy_slab, k_ppr_sum, k_count_above, bounds, select, k_index_alloc
        case EV_BATCH: f.batch_ms += ms; f.batches++; break;                          // a whole batch, from its reset to its close-out
        case EV_PUSH_ACCUM: f.push_accum_ms += ms; f.push_accum_launches++; break;    // k_accum of a push level
        case EV_WALK_ACCUM: f.walk_accum_ms += ms; break;                             // k_accum of the walk results (narrow layout)
        case EV_ROUND_SWEEP: f.push_accum_ms += ms; break;                            // k_round_sweep: part of the level's accumulate time, not a launch of its own in the counts
        case EV_PUSH_TAIL: f.push_tail_ms += ms; f.push_tail_launches++; break;       // k_push_tail
        case EV_PUSH_TEAM: f.push_team_ms += ms; f.push_team_launches++; break;       // k_push_team
        case EV_BWD: t.bwd_ms += ms; break;               // k_bwd_push: reported through fora_bwd_stats only (fora_timing keeps its layout)
        case EV_COMBINE: t.combine_ms += ms; break;       // BiPPR's transposes, combines and finish: fora_bwd_stats only
        case EV_SP_COMPACT: t.sp_compact_ms += ms; break; // k_sparse_count / k_sparse_write: reported through fora_sparse_stats only
        case EV_SEED_COMBINE: t.seed_combine_ms += ms; break; // k_seed_combine: reported through fora_seeds_stats only
        case EV_SW_COMPACT: t.sw_compact_ms += ms; break;     // the sweep's count / write / key passes: fora_sweep_stats only
        case EV_SW_SORT: t.sw_sort_ms += ms; break;           // k_sweep_sort_lds / k_sweep_sort_step: fora_sweep_stats only
        case EV_SW_CUT: t.sw_cut_ms += ms; break;             // scatter, k_sweep_cut, k_sweep_scan, reset: fora_sweep_stats only
        case EV_PROP_GATHER: t.prop_gather_ms += ms; break;   // k_prop_gather: fora_prop_stats only
        case EV_PROP_COMBINE: t.prop_combine_ms += ms; break; // k_prop_combine: fora_prop_stats only
        case EV_TK_SELECT: t.tk_select_ms += ms; break;       // k_topk_rows: fora_topk_stats only
        case EV_SDDMM: t.sddmm_ms += ms; break;               // k_prop_sddmm: fora_sddmm_stats only
        case EV_SOFTMAX: t.softmax_ms += ms; break;           // the k_softmax_* kernels of a call: fora_softmax_stats only
        case EV_ATTN: t.attn_ms += ms; break;                 // every launch of an ATTENTION call: fora_attn_stats only
        case EV_COLS: t.cols_ms += ms; break;                 // the bitmap's clear and the five k_cols_* kernels: fora_cols_stats only
        case EV_SUB: t.sub_ms += ms; break;                   // the k_sub_* kernels of a call: ms_out of fora_hip_sparse_subgraph only
        case EV_SUBP_T: t.subp_t_ms += ms; break;             // the transposition of the held subgraph: ms_out[0] of the SUBGRAPH PRODUCTS calls only
        case EV_SUBP_SHORT: t.subp_short_ms += ms; break;     // k_sub_agg: ms_out[1] of those calls only
        case EV_SUBP_LONG: t.subp_long_ms += ms; break;       // the gather and combine launches of their long rows: ms_out[2] only
        case EV_STORE: t.store_ms += ms; break;              // k_store_take; k_store_check and the copies of a put / load: fora_store_stats only
        case EV_PROPT_TRANSPOSE: t.propt_transpose_ms += ms; break; // the k_propt_* kernels and the host's prefix sum between them: fora_propt_stats only
        }
    }
    t.ev_used = 0;
}
// A call that fails leaves no pair behind (every entry point's last step): the next call's timings hold only its own launches.
void drop_pairs(fora_ctx *c) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->tm.ev_used = 0;
}
int drop_pairs_unless_ok(fora_ctx *c, int rc) { if (rc != FORA_OK && c && c->tm.ev_used) drop_pairs(c); return rc; }

int check_dev_err(fora_ctx *c) {
    uint32_t e = 0;
    HIPCHK(c, hipMemcpyAsync(&e, c->ws.d_err.get(), sizeof(e), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->retry.overflow = (e & ERR_BUCKET_OVERFLOW) != 0;
    c->team_run.timeout_seen = (e & ERR_TEAM_TIMEOUT) != 0;
    if (e) {
        c->team_run.dirty = true;
        char buf[256];
        snprintf(buf, sizeof(buf), "device work list overflow (flags 0x%x%s)", e,
                 (e & ERR_TEAM_TIMEOUT) ? ": a team of k_push_team waited too long for a member (workgroups not co-resident); the call is run again with the bucketed push"
                 : (e & ERR_BUCKET_OVERFLOW) ? ": message buckets and their overflow list are full, raise FORA_HIP_BKCAP" : "");
        return fail(c, FORA_E_OVERFLOW, buf);
    }
    return FORA_OK;
}

// ---- plumbing shared by the batch entry points
// first checks of every batch call: graph and params present, `nq` ids behind a non-null pointer
int check_batch_args(fora_ctx *c, const int32_t *ids, int nq, const char *what = "source") {
    if (!c) return FORA_E_ARG;
    if (!c->g.n) return fail(c, FORA_E_ARG, "set_graph first");
    if (!c->par.have) return fail(c, FORA_E_ARG, "set_params first");
    if (nq < 0 || (nq && !ids)) return fail(c, FORA_E_ARG, std::string("bad ") + what + "s: negative count or null array");
    return FORA_OK;
}
// ... and the last one, after the call's own arguments: every id in [0, n) (the ids are read only once all else passed)
int check_id_range(fora_ctx *c, const int32_t *ids, int nq, const char *what = "source") {
    for (int i = 0; i < nq; i++)
        if (ids[i] < 0 || ids[i] >= c->g.n) return fail(c, FORA_E_ARG, std::string(what) + " id out of range");
    return FORA_OK;
}
// k of a top-k output: what k_topk_select takes
int check_k(fora_ctx *c, int k) {
    if (k < 1 || k > SEL_MAXK || k > c->g.n) return fail(c, FORA_E_ARG, "k out of range (1 .. min(1024, n))");
    return FORA_OK;
}

bool is_dangling(const fora_ctx *c, int32_t s) { return c->g.h_row_ptr[(size_t)s + 1] == c->g.h_row_ptr[(size_t)s]; }

// a device (ids, scores) pair of B * k entries, grown on demand
int grow_pair(fora_ctx *c, int k, DevBuf<int32_t> &ids, DevBuf<double> &scores) {
    HIPCHK(c, ids.ensure((size_t)c->ws.B * k));
    HIPCHK(c, scores.ensure((size_t)c->ws.B * k));
    return FORA_OK;
}

// Slots [slot, slot + cnt) of a device slab into rows [row, row + cnt) of the caller's n-wide arrays (either may be null):
// raw u64, and f64 at 2^-frac.
int copy_slab_out(fora_ctx *c, const uint64_t *slab, uint64_t slot, uint64_t row, uint64_t cnt, uint64_t *fix_out, double *f64_out,
                  int frac) {
    const uint64_t n = (uint64_t)c->g.n, at = row * n, from = slot * n, len = cnt * n;
    if (fix_out) HIPCHK(c, hipMemcpy(fix_out + at, slab + from, len * 8, hipMemcpyDeviceToHost));
    if (f64_out) {
        // u64 and f64 have the same size: copy raw, convert in place on the host
        double *dst = f64_out + at;
        HIPCHK(c, hipMemcpy(dst, slab + from, len * 8, hipMemcpyDeviceToHost));
        const uint64_t *raw = (const uint64_t *)dst;
        for (uint64_t x = 0; x < len; x++) dst[x] = std::ldexp((double)raw[x], -frac);
    }
    return FORA_OK;
}

// The top k of slots [0, nb) (Workspace::d_topk_ids / d_topk_sc) into the caller's ids / scores (either may be null): slot i to row
// rows[i], or to row row0 + i without rows; the scores times `scale`.
int copy_topk_out(fora_ctx *c, int nb, int k, int32_t *ids, double *scores, uint64_t row0, const int *rows = nullptr, double scale = 1.0) {
    std::vector<int32_t> hid(ids ? (size_t)nb * k : 0);
    std::vector<double> hsc(scores ? (size_t)nb * k : 0);
    if (ids) HIPCHK(c, hipMemcpyAsync(hid.data(), c->ws.d_topk_ids.get(), hid.size() * 4, hipMemcpyDeviceToHost, c->stream));
    if (scores) HIPCHK(c, hipMemcpyAsync(hsc.data(), c->ws.d_topk_sc.get(), hsc.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the ctx stream does not synchronise with the null stream)
    for (int i = 0; i < nb; i++) {
        const uint64_t at = (rows ? (uint64_t)rows[i] : row0 + (uint64_t)i) * (uint64_t)k;
        if (ids) memcpy(ids + at, hid.data() + (size_t)i * k, (size_t)k * 4);
        if (scores) for (int j = 0; j < k; j++) scores[at + j] = hsc[(size_t)i * k + j] * scale;
    }
    return FORA_OK;
}

// End of a batch: close its event pair (null: none), read the device error word (waits for the stream), check the launches, collect the event
// times.  The batch pair spans functions and ends here, ahead of the error word's copy: ended by hand; its owner's destructor covers the early returns.
int close_batch(fora_ctx *c, EvSpan *batch, const char *what) {
    if (batch) batch->end();
    if (int rc = check_dev_err(c)) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, FORA_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    ev_collect(c);
    return FORA_OK;
}

// the per-slot counters of a batch (host copy of its QState words) into fora_timing
void fold_counters(fora_ctx *c, const QState *qs, int nb) {
    for (int i = 0; i < nb; i++) {
        c->tm.total.pops += qs[i].pops;
        c->tm.total.relax += qs[i].relax;
        c->tm.total.walks += qs[i].n_walks;
        c->tm.total.idx_hits += qs[i].n_hit;
    }
}

// Level loop of the push for the slots already initialised (level-0 frontier in place).
// Launches run ahead of the host by SPEC levels: an empty level costs a few near-empty
// launches, a host round trip per level would cost more.
// Frontier size (largest slot) from which k_push_tail takes over; 0: never.  ws, push of 1000 queries (round 2's
// tail kernel: no agent-scope fences, 4 relaxations in flight per lane): 1024: 86.3 ms, 4096: 85.2, 16384: 82.5,
// 32768: 81.9, 131072: 163 (one workgroup per slot cannot feed the peak levels)
// The tail runs one workgroup per slot, so it only pays while the slots alone fill the chip: with the 14 slots of a
// Twitter-2010-sized batch 32768 -> 2048 takes the tail from 128 ms to 11 ms per 28 queries (15.05 -> 15.81 q/s);
// LJ-sized, 140 slots: 32768 -> 4096 takes it from 16.8 to 2.2 ms per 280 queries (the bucketed levels it
// replaces cost less).  Default: 32 x the slot count, between 2048 and 32768.
static uint32_t tail_max_of(const fora_ctx *c, int nq) {
    return (uint32_t)(c->opt_.tail < 0 ? std::min<int64_t>(32768, std::max<int64_t>(2048, (int64_t)nq * 32)) : c->opt_.tail);
}
static inline size_t tail_lds(const Dev &d) { return d.tail_hubs && d.col_hub ? (size_t)d.hubs * 8 : 0; } // k_push_tail's dynamic LDS

// Wide accumulate: bins per workgroup (Dev::acc_group) and the grid's x size.  One bin per workgroup for query / power-iteration
// calls; the top-k drivers on wide graphs (many slots, rounds that touch a handful of bins: 94 k workgroups per launch at
// Twitter-2010 size, nearly all of them empty) take up to 8 consecutive bins of a slot per workgroup -- k_accum<false> 58 -> 39 ms
// per 125-source step, 301 -> 318 q/s.  (For LJ-sized queries, same 94 k workgroups but mostly busy ones: 211.7 ms grouped against
// 206.6 -- the bins of a group run one after the other --, hence not there.)
static unsigned acc_grid(const fora_ctx *c, Dev &dp, int nq) {
    const uint64_t pairs = (uint64_t)dp.bin_cnt * (uint64_t)std::max(1, nq);
    const uint64_t want = (uint64_t)std::max(1, c->prop.multiProcessorCount) * 24; // workgroups that keep the chip busy with one per CU at a time
    uint32_t g = c->retry.div > 1 ? (uint32_t)std::min<uint64_t>(std::max<uint64_t>(pairs / want, 1), 8) : 1u;
    if (c->opt_.acc_group > 0) g = (uint32_t)std::min<int64_t>(c->opt_.acc_group, ACC_GROUP_MAX);
    dp.acc_group = g;
    return (unsigned)((dp.bin_cnt + g - 1) / g);
}
int run_push_levels(fora_ctx *c, const Dev &d, uint64_t *levels_run = nullptr, int level_cap = 0, bool round_start = false) {
    const int nq = d.nq;
    const WsPlan &p = c->ws.plan;
    const uint32_t tail_max = tail_max_of(c, nq);
    if (round_start && p.binned && level_cap <= 0 && d.rounds <= 1 && c->opt_.tail != 0) {
        // A round of the top-k / --balanced drivers starts from every node at or over the round's threshold
        // (k_topk_frontier), often a handful: when no slot's frontier is larger than what k_push_tail takes over at anyway,
        // the whole round runs inside that kernel -- one launch instead of two per level plus the look-ahead levels
        // (Twitter-2010-sized top-k: 391 level launches of mostly empty workgroups per 125 queries).
        uint32_t *cnt = c->ws.h_flc.get();
        HIPCHK(c, hipMemcpyAsync(cnt, d.fl_count[0], (size_t)nq * 4 * CSTRIDE, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        uint32_t fmax = 0;
        for (int i = 0; i < nq; i++) fmax = std::max(fmax, cnt[(size_t)i * CSTRIDE]);
        if (fmax == 0) { if (levels_run) *levels_run = 0; return FORA_OK; }
        if (fmax <= tail_max) {
            EvSpan ev(c, EV_PUSH_TAIL);
            hipLaunchKernelGGL(k_push_tail, dim3(nq), dim3(TAIL_THREADS), tail_lds(d), c->stream, d, 0, 0);
            ev.end();
            c->tm.total.levels++;
            if (levels_run) *levels_run = 1;
            hipError_t e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return fail(c, FORA_E_HIP, std::string("push: ") + hipGetErrorString(e));
            e = hipGetLastError(); // (the launch check of the level loop's epilogue)
            if (e != hipSuccess) return fail(c, FORA_E_HIP, std::string("push launch: ") + hipGetErrorString(e));
            return FORA_OK;
        }
    }
    // the bin kernel has no instantiation for these: ensure_row_split builds split offsets for several passes only, which the narrow layout
    // and the hub copy (make_dev) never run
    if (p.binned && d.row_split && (d.col_hub || !d.wide)) return fail(c, FORA_E_ARG, "push: pass-split rows with a narrow layout or a hub copy");
    hipEvent_t done[SPEC + 1];
    for (auto &e : done) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    int rc = FORA_OK;
    int L = 0;
    const unsigned xb = p.binned ? p.sub : 1u; // producer workgroups per slot = sub-buckets per bucket (Dev::bk_w); ws at 1000 slots: 4 -> 196 ms, 8 -> 178, 16 -> 163, 32 -> 174
    bool past_peak = c->opt_.tail_always == 1; // tests: do not wait for the frontier to have been large first
    for (;; L++) {
        if (level_cap > 0 && L >= level_cap) break; // power iteration: a fixed number of levels
        if (L >= MAX_LEVELS) { rc = fail(c, FORA_E_OVERFLOW, "push level cap reached"); break; }
        if (p.binned) {
            for (int lo = 0; lo < p.nbins; lo += p.pbins) { // one pass per group of pbins bins (usually one)
                Dev dp = d;
                if (level_cap > 0 || d.rounds > 1) dp.defer_k = 0; // capped runs (power iteration) and threshold rounds keep plain levels
                dp.bin_lo = lo;
                dp.bin_cnt = std::min(p.pbins, p.nbins - lo);
                dp.pass = lo / p.pbins;
                dp.pop_next = !(level_cap > 0 && L + 1 >= level_cap); // a capped run leaves the last crossing nodes unpopped
                dp.launch_par = (int32_t)(c->bin_launches++ & 1);
                EvSpan ev(c, EV_PUSH_EXPAND);
                {
                    const size_t hub_lds = dp.col_hub ? (size_t)dp.hubs * 8 : 0;
                    const bool hub = dp.col_hub != nullptr, split = dp.row_split != nullptr, sched = TEST_PATHS && (dp.rounds > 1 || dp.defer_k > 0);
                    const dim3 bgrid = (dp.wide && (dp.slot_major & 1u)) ? dim3(nq, xb) : dim3(xb, nq); // (Dev::slot_major: the slot is the fastest-varying index)
#define FORA_BIN_LAUNCH(HUBV, SPLITV, SCHEDV, QUADV) hipLaunchKernelGGL((k_pushq_bin<NBV, HUBV, SPLITV, SCHEDV, QUADV>), bgrid, dim3(BinThreads<NBV>::value), hub_lds, c->stream, dp, L)
                    // Only the forms a plan can reach are instantiated (checked above: pass-split rows come with a wide layout and without the hub copy;
                    // make_dev sets col4 for wide layouts in one pass only).
                    auto pick = [&](auto nb) {
                        constexpr int NBV = decltype(nb)::value;
                        if constexpr (TEST_PATHS) if (sched) { FORA_BIN_LAUNCH(true, true, true, false); return; } // schedule experiments: the everything instantiation (test library only)
                        if constexpr (NBV > MAX_BINS) {
                            if (split) { FORA_BIN_LAUNCH(false, true, false, false); return; }
                            if (dp.col4) { if (hub) FORA_BIN_LAUNCH(true, false, false, true); else FORA_BIN_LAUNCH(false, false, false, true); return; }
                        }
                        if (hub) FORA_BIN_LAUNCH(true, false, false, false); else FORA_BIN_LAUNCH(false, false, false, false);
                    };
                    if (d.wide && p.pbins > MAX_BINS_WIDE) pick(std::integral_constant<int, MAX_BINS_HUGE>());
                    else if (d.wide) pick(std::integral_constant<int, MAX_BINS_WIDE>());
                    else pick(std::integral_constant<int, MAX_BINS>());
#undef FORA_BIN_LAUNCH
                }
                ev.begin(EV_PUSH_ACCUM);
                if (d.wide) { const unsigned gx = acc_grid(c, dp, nq); hipLaunchKernelGGL((k_accum<false, true>), (dp.slot_major & 2u) ? dim3(nq, gx) : dim3(gx, nq), dim3(ACC_THREADS_WIDE), 0, c->stream, dp, L); }
                else hipLaunchKernelGGL((k_accum<false, false>), dim3(dp.bin_cnt, nq), dim3(ACC_THREADS), 0, c->stream, dp, L);
            }
            if (TEST_PATHS && d.rounds > 1) { // threshold rounds: slots whose frontier ran dry move on to the next (halved) threshold
#if FORA_TEST_PATHS
                EvSpan ev(c, EV_ROUND_SWEEP);
                hipLaunchKernelGGL(k_round_sweep, dim3(std::min<uint32_t>(slab_grid_x(c, nq), 32u), nq), dim3(BLOCK), 0, c->stream, d, L);
#endif
            }
            (void)hipMemcpyAsync(c->ws.h_flc.get() + (size_t)((L + 1) % FLC_RING) * c->ws.B * CSTRIDE, d.fl_count[(L + 1) & 1],
                                 (size_t)nq * 4 * CSTRIDE, hipMemcpyDeviceToHost, c->stream);
        } else {
            EvSpan ev(c, EV_PUSH_POP);
            hipLaunchKernelGGL(k_push_pop, dim3(c->grid_blocks), dim3(BLOCK), 0, c->stream, d, L);
            ev.begin(EV_PUSH_EXPAND);
            hipLaunchKernelGGL(k_push_expand, dim3(c->grid_blocks), dim3(BLOCK), 0, c->stream, d, L);
            ev.end();
            (void)hipMemcpyAsync(c->ws.h_pinned.get() + L + 1, &d.wl_count[L + 1], sizeof(unsigned long long),
                                 hipMemcpyDeviceToHost, c->stream);
        }
        c->tm.total.levels++;
        (void)hipEventRecord(done[L % (SPEC + 1)], c->stream);
        if (L >= SPEC) {
            const int K = L - SPEC;
            if (hipEventSynchronize(done[K % (SPEC + 1)]) != hipSuccess) { rc = fail(c, FORA_E_HIP, "event sync"); break; }
            bool empty;
            uint32_t fmax = 0;
            if (p.binned) {
                empty = true;
                const uint32_t *cnt = c->ws.h_flc.get() + (size_t)((K + 1) % FLC_RING) * c->ws.B * CSTRIDE;
                uint32_t rounds_left = 0; // word 1 of a slot's counter line: threshold rounds still to come (k_round_sweep)
                for (int i = 0; i < nq; i++) { // word 2: nodes the level deferred (they are part of the work that is left)
                    fmax = std::max(fmax, cnt[(size_t)i * CSTRIDE] + cnt[(size_t)i * CSTRIDE + 2]);
                    rounds_left = std::max(rounds_left, cnt[(size_t)i * CSTRIDE + 1]);
                }
                empty = fmax == 0 && rounds_left == 0;
                if (rounds_left) fmax = std::max(fmax, tail_max + 1); // k_push_tail knows the final threshold only
            } else {
                empty = c->ws.h_pinned.get()[K + 1] == 0;
            }
            if (fmax > tail_max) past_peak = true; // the first levels are small too, but growing
            if (!empty && p.binned && tail_max > 0 && past_peak && fmax <= tail_max) {
                // every slot's frontier is small: finish inside one workgroup per slot instead of launching levels
                const int next = L + 1;
                const int remaining = level_cap > 0 ? level_cap - next : 0;
                if (level_cap <= 0 || remaining > 0) {
                    EvSpan ev(c, EV_PUSH_TAIL);
                    Dev dt = d;
                    if (d.rounds > 1) dt.defer_k = 0;
                    hipLaunchKernelGGL(k_push_tail, dim3(nq), dim3(TAIL_THREADS), tail_lds(dt), c->stream, dt, next, remaining);
                    ev.end();
                    c->tm.total.levels++;
                }
                break;
            }
            if (empty) break;
        }
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    for (auto &ev : done) (void)hipEventDestroy(ev);
    if (levels_run) *levels_run = (uint64_t)L + 1;
    if (rc == FORA_OK && e != hipSuccess) rc = fail(c, FORA_E_HIP, std::string("push: ") + hipGetErrorString(e));
    if (rc == FORA_OK) {
        e = hipGetLastError();
        if (e != hipSuccess) rc = fail(c, FORA_E_HIP, std::string("push launch: ") + hipGetErrorString(e));
    }
    return rc;
}

// Team push of a batch (fora_team.h): ONE launch runs every slot's push down to a small frontier with the residue
// resident in LDS, k_push_tail finishes the slots.  Nothing here waits for the device.
static bool use_team(const fora_ctx *c, const Dev &d) {
    // not after a time-out
    return c->g.team.T && c->ws.d_team_msg && c->ws.plan.binned && !d.wide && !c->bal.on && d.rounds <= 1 && d.defer_k == 0 && want_team(c) &&
           c->ws.team_fit != 0 && c->team_run.suspend == 0;
}
// Can every workgroup of a k_push_team launch be resident at once?  (Asked once per workspace, the one being built with its
// team buffers in place; raises the kernel's dynamic LDS limit on the way.)
int team_fits(fora_ctx *c, Workspace &w) {
    const size_t lds = ((size_t)c->g.team.R + 1 + c->g.team.H) * 8;
    hipFuncAttributes fa{};
    HIPCHK(c, hipFuncGetAttributes(&fa, (const void *)k_push_team));
    HIPCHK(c, hipFuncSetAttribute((const void *)k_push_team, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(163840 - (int)fa.sharedSizeBytes)));
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_push_team, TEAM_THREADS, lds) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
    const uint32_t grid = w.team_n * c->g.team.T;
    w.team_fit = (uint64_t)per_cu * (uint64_t)c->prop.multiProcessorCount >= grid ? 1 : 0;
    int coop = 0;
    if (hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, c->device) != hipSuccess) { (void)hipGetLastError(); coop = 0; }
    c->team_run.coop_ok = c->opt_.team_coop == 1 && coop != 0;
    return FORA_OK;
}
int run_push_team(fora_ctx *c, const Dev &d) {
    const uint32_t T = c->g.team.T, nteams = c->ws.team_n;
    TeamDev a{};
    a.n = d.n; a.nq = d.nq; a.rowinfo = d.rowinfo; a.row_ptr = d.row_ptr; a.deg = d.deg; a.src = d.src;
    a.residue = d.residue; a.ppr = d.ppr; a.fl0 = d.fl[0]; a.fl_count0 = d.fl_count[0]; a.inc_tab0 = d.inc_tab[0];
    a.segq_cap = d.segq_cap; a.qs = d.qs; a.err = d.err; a.afix = d.afix; a.t1 = d.t1;
    a.T = T; a.R = c->g.team.R; a.nteams = nteams;
    a.colt = c->g.team.d_colt.get(); a.rowq = c->g.team.d_rowq.get(); a.n2l = c->g.team.d_n2l.get(); a.l2n = c->g.team.d_l2n.get(); a.deg16 = c->g.team.d_deg16.get(); a.rowl = c->g.team.d_rowl.get(); a.rsvl = c->ws.d_team_rsvl.get(); a.rlog_id = c->ws.d_team_rlog_id.get(); a.rlog_val = c->ws.d_team_rlog_val.get(); a.rlog_cap = c->opt_.team_log == 0 ? 0u : c->opt_.team_log > 0 ? std::min<uint32_t>((uint32_t)c->opt_.team_log, c->ws.plan.team_rlog_cap) : c->ws.plan.team_rlog_cap; a.H = c->g.team.H; a.hubtgt = c->g.team.d_hubtgt.get(); a.off = c->g.team.d_off.get(); a.msg = c->ws.d_team_msg.get(); a.inct = c->ws.d_team_inct.get(); a.cntw = c->ws.d_team_cnt.get();
    const Workspace &w = c->ws;
    const TeamCtl ctl = team_ctl_layout(nteams, w.B);
    a.ctl = w.d_team_ctl.get(); a.sync = (unsigned long long *)(a.ctl + ctl.sync); a.slot_seq = a.ctl + ctl.slot_seq;
    // frontier size of a slot at which k_push_tail (one workgroup per slot, global atomics) takes over; 0: never
    const int64_t tail_auto = 4096;
    a.tail_max = (uint32_t)std::min<int64_t>(std::max<int64_t>(c->opt_.team_tail < 0 ? tail_auto : c->opt_.team_tail, 0), 0x7FFFFFFF);
    if (c->opt_.tail == 0) a.tail_max = 0; // `tail` 0 keeps k_push_tail out of every path (tests)
    a.tail_always = c->opt_.tail_always == 1 ? 1u : 0u;
    const uint32_t grid = nteams * T;
    a.xcd = (c->opt_.team_xcd >= 1 && grid % 8 == 0 && (grid / 8) % T == 0) ? (uint32_t)c->opt_.team_xcd : 0u;
    a.stamps = c->d_stamps.get();
    a.abort_level = (uint32_t)std::min<int64_t>(std::max<int64_t>(c->opt_.team_abort_level, 0), 1 << 20);
    a.timeout_ticks = (uint64_t)std::min<int64_t>(std::max<int64_t>(c->opt_.team_timeout_ms, 0), 60000) * 100000ull; // (100 MHz wall clock)
    const size_t lds = ((size_t)a.R + 1 + a.H) * 8;
    if (c->team_run.dirty) { HIPCHK(c, w.d_team_rsvl.zero(c->stream)); c->team_run.dirty = false; }
    HIPCHK(c, w.d_team_ctl.zero(c->stream, ctl.slot_seq)); // the words before the slot sequences
    HIPCHK(c, w.d_team_cnt.zero(c->stream)); // no barrier tag of an earlier launch
    HIPCHK(c, w.d_team_ctl.fill(c->stream, 0xFF, ctl.slot_seq, (size_t)nteams * ((size_t)d.nq + 2)));
    EvSpan ev(c, EV_PUSH_TEAM);
    // The members of a team spin on each other: every workgroup of the launch must be resident at once.  team_fits() has
    // checked that the grid fits the device; a cooperative launch makes the runtime promise it (and keeps cooperative
    // kernels of other contexts from interleaving their workgroups with ours).  Whatever still goes wrong ends in
    // ERR_TEAM_TIMEOUT after team_timeout_ms, and with_retry runs the call again through the bucketed kernels.
    bool launched = false;
    if (c->team_run.coop_ok && !c->team_run.coop_failed) {
        void *args[] = {(void *)&a};
        const hipError_t le = hipLaunchCooperativeKernel((const void *)k_push_team, dim3(grid), dim3(TEAM_THREADS), args, (unsigned)lds, c->stream);
        if (le == hipSuccess) launched = true;
        else { (void)hipGetLastError(); c->team_run.coop_failed = true; }
    }
    if (!launched) hipLaunchKernelGGL(k_push_team, dim3(grid), dim3(TEAM_THREADS), lds, c->stream, a);
    ev.end();
    c->tm.total.levels++;
    if (a.tail_max) {
        ev.begin(EV_PUSH_TAIL);
        hipLaunchKernelGGL(k_push_tail, dim3(d.nq), dim3(TAIL_THREADS), tail_lds(d), c->stream, d, 0, 0);
        ev.end();
        c->tm.total.levels++;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, FORA_E_HIP, std::string("team push launch: ") + hipGetErrorString(e));
    return FORA_OK;
}

// k_topk_select over the slabs of `ds.ppr`; large graphs first compact each slot's non-zero entries (in id order, so
// ties keep resolving to the lowest ids) into the push's frontier / increment buffers, which are idle here.
constexpr unsigned NZ_X = 1024;
int launch_select(fora_ctx *c, const Dev &ds, int nb, int k, int32_t *ids, double *scores, int raw, const double *h_thr = nullptr) {
    bool compact = c->ws.plan.binned && c->g.n >= (1 << 20);
    if (c->opt_.select_compact >= 0) compact = c->ws.plan.binned && c->opt_.select_compact == 1; // tests: force / forbid the compacted form
    if (!compact) {
        hipLaunchKernelGGL(k_topk_select, dim3(nb), dim3(SEL_THREADS), 0, c->stream, ds, k, ids, scores, raw,
                           (const uint32_t *)nullptr, (const uint64_t *)nullptr, (const uint32_t *)nullptr);
        return FORA_OK;
    }
    HIPCHK(c, c->ws.d_nz_counts.ensure((size_t)c->ws.B * (NZ_X + 1)));
    const unsigned X = (unsigned)std::min<uint64_t>(NZ_X, ((uint64_t)c->g.n + 4095) / 4096);
    const uint32_t R = (uint32_t)(((uint64_t)c->g.n + X - 1) / X);
    uint32_t *ccount = c->ws.d_nz_counts.get() + (size_t)c->ws.B * NZ_X;
    const double *thr = nullptr; // per-slot lower limit of the entries worth compacting (see k_nz_count)
    if (h_thr && !raw) {
        HIPCHK(c, c->ws.d_sel_thr.ensure((size_t)c->ws.B));
        HIPCHK(c, hipMemcpyAsync(c->ws.d_sel_thr.get(), h_thr, (size_t)nb * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); // h_thr is the caller's pageable buffer
        thr = c->ws.d_sel_thr.get();
    }
    hipLaunchKernelGGL(k_nz_count, dim3(X, nb), dim3(BLOCK), 0, c->stream, ds, R, c->ws.d_nz_counts.get(), thr);
    hipLaunchKernelGGL(k_nz_write, dim3(X, nb), dim3(BLOCK), 0, c->stream, ds, R, (const uint32_t *)c->ws.d_nz_counts.get(), c->ws.d_fl[0].get(),
                       c->ws.d_inc_tab[0].get(), ccount, thr);
    hipLaunchKernelGGL(k_topk_select, dim3(nb), dim3(SEL_THREADS), 0, c->stream, ds, k, ids, scores, raw,
                       (const uint32_t *)c->ws.d_fl[0].get(), (const uint64_t *)c->ws.d_inc_tab[0].get(), (const uint32_t *)ccount);
    return FORA_OK;
}

// per-level bookkeeping of the bucketed push that must start from zero
int reset_binned_counters(fora_ctx *c) {
    if (!c->ws.plan.binned) return FORA_OK;
    const Workspace &w = c->ws;
    HIPCHK(c, w.d_fl_count.zero(c->stream));
    HIPCHK(c, w.d_bk_count.zero(c->stream));
    HIPCHK(c, w.d_ov_count.zero(c->stream));
    HIPCHK(c, w.d_ov_bin.zero(c->stream));
    if (TEST_PATHS) { // bounded deferral's bitmaps and flags (test library only; 385 MB per top-k round at Twitter-2010 size)
        HIPCHK(c, w.d_dbm.zero(c->stream)); // (a complete push leaves them clear; an aborted one may not)
        HIPCHK(c, w.d_dflag.zero(c->stream));
    }
    HIPCHK(c, w.d_tile_ctr.zero(c->stream)); // both parity sets, every slot: a launch only re-zeroes the slots it runs
    return FORA_OK;
}

int reset_batch_state(fora_ctx *c, int nq, const int32_t *sources) {
    const uint64_t slabs = (uint64_t)nq * c->g.n; // the slabs of the batch's slots only
    EvSpan ev(c, EV_OTHER);
    HIPCHK(c, c->ws.d_residue.zero(c->stream, slabs));
    HIPCHK(c, c->ws.d_ppr.zero(c->stream, slabs));
    HIPCHK(c, c->ws.d_counters.zero(c->stream));
    HIPCHK(c, c->ws.d_err.zero(c->stream));
    HIPCHK(c, c->ws.d_wit_count.zero(c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ws.d_src.get(), sources, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    return reset_binned_counters(c); // (the span ends behind it)
}

enum { RUN_PUSH_ONLY = 1 };

// slots per batch for nq queries on B slots: the fewest batches, all about the same size (1000 queries on 140 slots: 8 x 125,
// not 7 x 140 + 20 -- a small trailing batch costs almost a full batch's level latencies)
static int even_batch(int nq, int B) {
    if (nq <= B || B <= 0) return std::max(nq, 1);
    const int nbatch = (nq + B - 1) / B;
    return (nq + nbatch - 1) / nbatch;
}

// ---- held rows (the comment above CountBufs): what the sparse rows and the sweep profiles share of one attempt of a call
struct RowsRun {
    uint64_t thr = 1;
    CompactGeom geo; RowLayout lay; // the compaction's ids per workgroup, workgroups per slot; where the rows lie
};

// what every entry point that makes a held result starts with: the held one ends here, whatever becomes of this call
// (k: of a top-k call, checked beside the threshold -- a bad one ends the held result like a bad threshold)
int held_rows_begin(fora_ctx *c, HeldRows &held, const int64_t *row_ptr, double threshold, uint64_t &thr, const int64_t *k = nullptr) {
    if (&held == static_cast<HeldRows *>(&c->sp)) sparse_unheld(c);
    held.valid = false; held.entries = 0;
    if (!row_ptr) return fail(c, FORA_E_ARG, "row_ptr is required");
    if (!threshold_ok(threshold)) return fail(c, FORA_E_ARG, "threshold above 1 or not a number");
    if (k && !topk_k_ok(*k)) return fail(c, FORA_E_ARG, "k below 1");
    thr = threshold_word(threshold);
    return FORA_OK;
}

// the compaction's geometry, and the count buffers for batches of at most `slots` slots
int prepare_counts(fora_ctx *c, RowsRun &r, CountBufs &cb, int slots) {
    r.geo = compact_geom((uint64_t)c->g.n);
    HIPCHK(c, cb.d_counts.ensure((size_t)slots * r.geo.X));
    HIPCHK(c, cb.d_tot.ensure((size_t)slots));
    HIPCHK(c, cb.h_tot.ensure((size_t)slots));
    return FORA_OK;
}

// count pass over nb rows; the counts are in cb.h_tot once the stream has been synchronised.
// rows: where the nb rows lie, n words each, 16-byte aligned (null: the workspace's ppr slabs)
int count_rows(fora_ctx *c, const RowsRun &r, const uint64_t *rows, int nb, const CountBufs &cb, EvKind kind) {
    HIPCHK(c, hipMemsetAsync(cb.d_tot.get(), 0, (size_t)nb * 4, c->stream));
    EvSpan ev(c, kind);
    hipLaunchKernelGGL(k_sparse_count, dim3(r.geo.X, nb), dim3(BLOCK), 0, c->stream, rows ? rows : (const uint64_t *)c->ws.d_ppr.get(), (uint32_t)c->g.n, r.thr, r.geo.R,
                       cb.d_counts.get(), cb.d_tot.get());
    ev.end();
    HIPCHK(c, hipMemcpyAsync(cb.h_tot.get(), cb.d_tot.get(), (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    return FORA_OK;
}

// room in every held array for the entries placed so far; what the device has written of them is kept (grow_guess: the
// rows still to come are guessed at).  No room: the held arrays go, and drop_rest (if any) frees what else goes with them.
template <typename... T>
int reserve_rows(fora_ctx *c, const RowLayout &lay, const char *no_room, void (*drop_rest)(fora_ctx *), DevBuf<T> &...held) {
    const uint64_t need = lay.cur;
    if (need <= std::min({(uint64_t)held.size()...})) return FORA_OK;
    const uint64_t keep = std::min({lay.written, (uint64_t)held.size()...});
    return [&](DevBuf<T>... grown) -> int { // the new arrays: moved in at the end, freed on every other way out
        for (uint64_t cap = grow_guess(need, (uint64_t)lay.next_row, (uint64_t)lay.nq);; cap = need) { // (a guess that does not fit is no reason to fail)
            if (((grown.alloc(cap) == hipSuccess) && ...)) break;
            (void)hipGetLastError(); (grown.reset(), ...);
            if (cap == need) {
                (void)hipStreamSynchronize(c->stream);
                (held.reset(), ...);
                if (drop_rest) drop_rest(c);
                return fail(c, FORA_E_NOMEM, no_room);
            }
        }
        if (keep) {
            const auto copy = [&](void *to, const void *from, size_t bytes) { HIPCHK(c, hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToDevice, c->stream)); return (int)FORA_OK; };
            int rc = FORA_OK;
            ((rc = rc ? rc : copy(grown.get(), held.get(), keep * sizeof(T))), ...);
            if (rc) return rc;
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        ((held = std::move(grown)), ...);
        return FORA_OK;
    }(DevBuf<T>()...);
}

// end of a call whose batches all went through, behind the layout's finish and the kind's reserve: the dangling rows'
// entries (single(count, entries, sources) launches the kind's kernel for them), the last event times, the result is held
template <typename Single> int finish_rows(fora_ctx *c, const RowLayout &lay, HeldRows &held, const char *what, int64_t *row_ptr, Single single) {
    DevBuf<int64_t> at; DevBuf<int32_t> src; // (freed on every return path)
    const size_t nd = lay.dang_at.size();
    if (nd) {
        HIPCHK(c, at.alloc(nd));
        HIPCHK(c, src.alloc(nd));
        HIPCHK(c, hipMemcpyAsync(at.get(), lay.dang_at.data(), nd * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(src.get(), lay.dang_src.data(), nd * 4, hipMemcpyHostToDevice, c->stream));
        single((uint32_t)nd, (const int64_t *)at.get(), (const int32_t *)src.get());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, FORA_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    ev_collect(c);
    held.entries = lay.cur; held.valid = true;
    if (&held == static_cast<HeldRows *>(&c->sp)) c->sparse_gen++;
    memcpy(row_ptr, lay.row_ptr.data(), ((size_t)lay.nq + 1) * 8);
    return FORA_OK;
}

// ---- sparse results (fora_hip_query_sparse_batch): what is their own
struct SparseRun : RowsRun {
    int live_done = 0;     // live rows written so far: d_base holds the first entry of each
    int64_t topk = 0;      // > 0: a top-k call, a row holds min(len, topk) entries (topk_place)
    TopkSums tk;
};

// per-call buffers of the two passes: `slots` slots per batch, `live` live rows in all
int sparse_prepare(fora_ctx *c, SparseRun &sp, int slots, int live) {
    if (int rc = prepare_counts(c, sp, c->sp.cnt, slots)) return rc;
    HIPCHK(c, c->sp.d_base.ensure((size_t)live));
    return FORA_OK;
}

int sparse_reserve(fora_ctx *c, const RowLayout &lay) { // (no room: the whole result goes)
    return reserve_rows(c, lay, "no device memory for the sparse result", free_sparse, c->sp.d_ids, c->sp.d_fix);
}

// k_topk_rows<true> stages up to TOPK_LDS_MAX words: its dynamic LDS limit is raised to what a CU has, once per context
int topk_lds_limit(fora_ctx *c) {
    if (c->topk_lds_ready) return FORA_OK;
    hipFuncAttributes fa{};
    HIPCHK(c, hipFuncGetAttributes(&fa, (const void *)k_topk_rows<true>));
    HIPCHK(c, hipFuncSetAttribute((const void *)k_topk_rows<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(163840 - (int)fa.sharedSizeBytes)));
    c->topk_lds_ready = true;
    return FORA_OK;
}

// sparse_place of a top-k call (the SPARSE RESULTS, TOP-K contract; planning in fora_topk_plan.h, kernels in
// fora_sparse_topk.h).  The counts give every row's held length min(len, k) and so its place in the held arrays before
// anything is written.  The batch is then written in pieces: k_sparse_write compacts a chunk of consecutive rows into the
// candidate scratch, k_topk_rows copies or selects every row of the chunk into its place, and the next chunk reuses the
// scratch behind them on the stream.  Every row goes through the scratch, the ones that keep everything too.
int topk_place(fora_ctx *c, SparseRun &sp, const int *at, int r0, int nb, const uint64_t *rows) {
    SparseResult &s = c->sp;
    const uint32_t *len = s.cnt.h_tot.get();
    const uint64_t n = (uint64_t)c->g.n;
    const uint32_t lds_cap = topk_lds_cap(c->opt_.topk_lds_cap);
    std::vector<uint64_t> out((size_t)nb);
    uint64_t total = 0, longest = 0;
    sp.lay.begin_batch();
    for (int i = 0; i < nb; i++) {
        out[(size_t)i] = (uint64_t)sp.lay.place(at ? at[i] : r0 + i, len[i], topk_held(len[i], sp.topk));
        sp.tk.add_row(len[i], topk_tier(len[i], sp.topk, lds_cap));
        total += len[i]; longest = std::max<uint64_t>(longest, len[i]);
    }
    if (int rc = sparse_reserve(c, sp.lay)) return rc;
    if (!total) return FORA_OK;
    // the scratch
    uint64_t free_entries = std::min(s.d_cand_ids.size(), s.d_cand_fix.size());
    if (c->opt_.topk_cand <= 0) {
        size_t fr = 0, tot = 0;
        HIPCHK(c, hipMemGetInfo(&fr, &tot));
        free_entries += (uint64_t)fr / 2 / (sizeof(int32_t) + sizeof(uint64_t)); // half of what is free: the held arrays may still grow
    }
    const uint64_t cand_cap = topk_cand_cap(c->opt_.topk_cand, free_entries, total, longest);
    if (s.d_cand_ids.ensure(cand_cap) != hipSuccess || s.d_cand_fix.ensure(cand_cap) != hipSuccess) {
        (void)hipGetLastError();
        s.d_cand_ids.reset(); s.d_cand_fix.reset();
        return fail(c, FORA_E_NOMEM, "no device memory for the top-k candidates: lower the option topk_cand");
    }
    const uint64_t ccap = std::min(s.d_cand_ids.size(), s.d_cand_fix.size()), hcap = std::min(s.d_ids.size(), s.d_fix.size());
    const TopkBatchPlan plan = topk_chunks(len, nb, cand_cap);
    const uint64_t *base = rows ? rows : (const uint64_t *)c->ws.d_ppr.get();
    std::vector<uint64_t> pack;
    std::vector<TopkRow> staged, plain; // rows selected in LDS; rows copied or selected from global memory
    for (const TopkChunk &ch : plan.chunks) {
        sp.tk.chunks++;
        if (!ch.entries) continue;
        const int q0 = topk_launch_row(ch.r0, n), nw = ch.r1 - q0;
        staged.clear(); plain.clear();
        pack.assign((size_t)nw, ccap); // write bases; a row in front of the chunk writes nothing
        uint32_t stage = 0;
        for (int i = ch.r0; i < ch.r1; i++) {
            pack[(size_t)(i - q0)] = plan.cand[(size_t)i];
            if (!len[i]) continue;
            const TopkRow r{plan.cand[(size_t)i], out[(size_t)i], len[i], (uint32_t)topk_held(len[i], sp.topk)};
            if (topk_tier(len[i], sp.topk, lds_cap) == TOPK_LDS) { staged.push_back(r); stage = std::max(stage, len[i]); }
            else plain.push_back(r);
        }
        const size_t at_staged = pack.size(), at_plain = at_staged + staged.size() * 3;
        pack.resize(at_plain + plain.size() * 3);
        if (!staged.empty()) memcpy(pack.data() + at_staged, staged.data(), staged.size() * sizeof(TopkRow));
        if (!plain.empty()) memcpy(pack.data() + at_plain, plain.data(), plain.size() * sizeof(TopkRow));
        HIPCHK(c, s.d_tkdesc.ensure(pack.size()));
        HIPCHK(c, hipMemcpyAsync(s.d_tkdesc.get(), pack.data(), pack.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); // (pageable source)
        if (!staged.empty()) if (int rc = topk_lds_limit(c)) return rc;
        EvSpan ev(c, EV_SP_COMPACT);
        hipLaunchKernelGGL(k_sparse_write, dim3(sp.geo.X, (unsigned)nw), dim3(BLOCK), 0, c->stream, base + (uint64_t)q0 * n, (uint32_t)n, sp.thr, sp.geo.R,
                           (const uint32_t *)s.cnt.d_counts.get() + (size_t)q0 * sp.geo.X, reinterpret_cast<const int64_t *>(s.d_tkdesc.get()),
                           s.d_cand_ids.get(), s.d_cand_fix.get(), ccap);
        ev.begin(EV_TK_SELECT);
        if (!staged.empty())
            hipLaunchKernelGGL(k_topk_rows<true>, dim3((unsigned)staged.size()), dim3(TOPK_BLOCK), (size_t)stage * 8, c->stream,
                               reinterpret_cast<const TopkRow *>(s.d_tkdesc.get() + at_staged), (const int32_t *)s.d_cand_ids.get(), (const uint64_t *)s.d_cand_fix.get(), ccap,
                               s.d_ids.get(), s.d_fix.get(), hcap);
        if (!plain.empty())
            hipLaunchKernelGGL(k_topk_rows<false>, dim3((unsigned)plain.size()), dim3(TOPK_BLOCK), 0, c->stream,
                               reinterpret_cast<const TopkRow *>(s.d_tkdesc.get() + at_plain), (const int32_t *)s.d_cand_ids.get(), (const uint64_t *)s.d_cand_fix.get(), ccap,
                               s.d_ids.get(), s.d_fix.get(), hcap);
    }
    return FORA_OK;
}

// write pass of the batch just closed (slot i: row at[i] of the caller; at null: row r0 + i); the slabs hold it until the
// next batch starts on the same stream.  rows: as for count_rows
int sparse_place(fora_ctx *c, SparseRun &sp, const int *at, int r0, int nb, const uint64_t *rows = nullptr) {
    if (sp.topk) return topk_place(c, sp, at, r0, nb, rows);
    std::vector<int64_t> base((size_t)nb);
    sp.lay.begin_batch();
    for (int i = 0; i < nb; i++) {
        const uint64_t len = c->sp.cnt.h_tot.get()[i];
        base[(size_t)i] = sp.lay.place(at ? at[i] : r0 + i, len, len);
    }
    if (int rc = sparse_reserve(c, sp.lay)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->sp.d_base.get() + sp.live_done, base.data(), (size_t)nb * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (`base` goes out of scope)
    EvSpan ev(c, EV_SP_COMPACT);
    hipLaunchKernelGGL(k_sparse_write, dim3(sp.geo.X, nb), dim3(BLOCK), 0, c->stream, rows ? rows : (const uint64_t *)c->ws.d_ppr.get(), (uint32_t)c->g.n, sp.thr, sp.geo.R,
                       (const uint32_t *)c->sp.cnt.d_counts.get(), (const int64_t *)(c->sp.d_base.get() + sp.live_done), c->sp.d_ids.get(), c->sp.d_fix.get(), (uint64_t)c->sp.d_ids.size());
    sp.live_done += nb;
    return FORA_OK;
}

int sparse_finish(fora_ctx *c, SparseRun &sp, int64_t *row_ptr, fora_sparse_stats *out, fora_topk_stats *tk = nullptr) {
    sp.lay.finish();
    if (int rc = sparse_reserve(c, sp.lay)) return rc; // (only grows when dangling rows came last)
    if (int rc = finish_rows(c, sp.lay, c->sp, "sparse result", row_ptr, [&](uint32_t nd, const int64_t *at, const int32_t *src) {
            hipLaunchKernelGGL(k_sparse_single, dim3((nd + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, nd, at, src,
                               c->sp.d_ids.get(), c->sp.d_fix.get(), (uint64_t)c->sp.d_ids.size());
        })) return rc;
    if (out) {
        memset(out, 0, sizeof(*out));
        out->entries = sp.lay.cur; out->max_row = sp.lay.max_row; out->thr_fix = sp.thr; out->batches = sp.lay.batches;
        out->compact_ms = c->tm.sp_compact_ms;
        if (sp.topk) out->max_row = topk_held(sp.lay.max_row, sp.topk); // the longest HELD row
    }
    if (tk) {
        memset(tk, 0, sizeof(*tk));
        tk->support = sp.tk.support; tk->max_support = sp.tk.max_support; tk->k = (uint64_t)sp.topk;
        tk->cut_rows = sp.tk.cut_rows; tk->lds_rows = sp.tk.lds_rows; tk->global_rows = sp.tk.global_rows; tk->chunks = sp.tk.chunks;
        tk->select_ms = c->tm.tk_select_ms;
    }
    return FORA_OK;
}

// ---- sweep cut (fora_hip_sweep_batch; the SWEEP CUT contract of include/fora_hip.h, kernels in fora_sweep.h): host side of
// one attempt of a call.  The profiles are laid out in the caller's order like the rows of a sparse result; a batch's rows are
// compacted, sorted and swept once the batch has closed -- its slabs hold the rows until the next batch starts on the stream.
static fora_sweep_row sweep_row_of(int64_t len, int64_t best, uint64_t cut, uint64_t vol, uint64_t den) {
    fora_sweep_row r;
    r.len = len; r.best = best; r.cut = cut; r.vol = vol; r.den = den;
    r.conductance = best ? (double)cut / (double)den : 1.0;
    return r;
}
struct SweepRun : RowsRun { // (lay.row_ptr: prefix sums of L)
    int64_t max_size = 0;
    std::vector<fora_sweep_row> rows; // nq
    int global_rows = 0; uint64_t edges = 0;
    SweepRun(uint64_t thr_, int64_t max_size_, int nq) : max_size(max_size_) {
        thr = thr_;
        rows.assign((size_t)std::max(nq, 0), sweep_row_of(1, 0, 0, 0, 0)); // a batch writes the row of every source it runs: a row none has written is a dangling source's
    }
};

// the rank block of min(live, sweep_rows) slabs, all -1
int sweep_prepare_rank(fora_ctx *c, int live) {
    SweepResult &w = c->swp;
    const uint64_t n = (uint64_t)c->g.n;
    const uint32_t rows = (uint32_t)std::min<int64_t>(live, c->opt_.sweep_rows > 0 ? c->opt_.sweep_rows : 256);
    const bool fresh = !w.d_rank || w.d_rank.size() < (uint64_t)rows * n;
    if (fresh && w.d_rank.alloc((uint64_t)rows * n) != hipSuccess) {
        (void)hipGetLastError();
        free_workspace(c); // (no room beside a workspace that is already there: that one goes, as for the seed sets' block)
        if (w.d_rank.alloc((uint64_t)rows * n) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, FORA_E_NOMEM, "no device memory for the sweep's rank block (sweep_rows x n words): lower the option sweep_rows");
        }
    }
    if (fresh || w.rank_dirty) HIPCHK(c, w.d_rank.fill(c->stream, 0xFF, 0, w.d_rank.size()));
    w.rank_dirty = false;
    w.rank_rows = rows;
    return FORA_OK;
}

// per-call buffers of the passes over a batch of at most `slots` slots
int sweep_prepare(fora_ctx *c, SweepRun &sw, int slots) {
    if (int rc = prepare_counts(c, sw, c->swp.cnt, slots)) return rc;
    HIPCHK(c, c->swp.d_out.ensure((size_t)slots));
    HIPCHK(c, c->swp.h_out.ensure((size_t)slots));
    return FORA_OK;
}

int sweep_reserve(fora_ctx *c, const RowLayout &lay) {
    return reserve_rows(c, lay, "no device memory for the sweep profiles", nullptr, c->swp.d_ids, c->swp.d_cut, c->swp.d_vol);
}

// the batch just closed (slot i: row at[i] of the caller; at null: row r0 + i): compaction, sort, and chunk by chunk the cut
// count and the scan.  rows: as for count_rows
int sweep_rows_of_batch(fora_ctx *c, SweepRun &sw, const int *at, int r0, int nb, const uint64_t *rows = nullptr) {
    SweepResult &w = c->swp;
    const uint32_t n = (uint32_t)c->g.n;
    const uint64_t *ppr = rows ? rows : c->ws.d_ppr.get();
    const auto row_of = [&](int i) { return at ? at[i] : r0 + i; };
    if (int rc = count_rows(c, sw, rows, nb, w.cnt, EV_SW_COMPACT)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    EvSpan ev(c);
    // layout: padded copies in the sort buffers, profiles in the held arrays (fora_sweep_plan.h)
    const uint32_t T = sweep_tile(c->opt_.sweep_lds_cap);
    const SweepBatchPlan plan = sweep_batch_plan(w.cnt.h_tot.get(), nb, sw.max_size, T, sw.lay, at, r0);
    const std::vector<SweepTile> &tiles = plan.tiles;
    const std::vector<SweepGRow> &grows = plan.grows;
    const uint32_t maxP = plan.maxP, maxL = plan.maxL;
    sw.global_rows += (int)grows.size();
    if (int rc = sweep_reserve(c, sw.lay)) return rc;
    if (w.d_tids.ensure(std::max<uint64_t>(plan.tneed, 1)) != hipSuccess || w.d_tkey.ensure(std::max<uint64_t>(plan.tneed, 1)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, FORA_E_NOMEM, "no device memory for the sweep's sort buffers");
    }
    const uint64_t tcap = std::min(w.d_tids.size(), w.d_tkey.size()), hcap = w.d_ids.size();
    HIPCHK(c, w.d_desc.ensure(std::max<size_t>(plan.pack.size(), 1)));
    HIPCHK(c, hipMemcpyAsync(w.d_desc.get(), plan.pack.data(), plan.pack.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (pageable source)
    const SweepDescView<const uint64_t> dv = plan.view<const uint64_t>(w.d_desc.get());
    const SweepRowDesc *d_rd = dv.rows();
    const int64_t *d_base = dv.tbase();
    const SweepTile *d_tiles = dv.tiles();
    const SweepGRow *d_grows = dv.grows();
    const auto gx = [](uint64_t items) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + BLOCK - 1) / BLOCK, 128)); };
    if (maxP) {
        ev.begin(EV_SW_COMPACT);
        hipLaunchKernelGGL(k_sparse_write, dim3(sw.geo.X, nb), dim3(BLOCK), 0, c->stream, ppr, n, sw.thr, sw.geo.R, (const uint32_t *)w.cnt.d_counts.get(), d_base,
                           w.d_tids.get(), w.d_tkey.get(), tcap);
        hipLaunchKernelGGL(k_sweep_keys, dim3(gx(maxP), nb), dim3(BLOCK), 0, c->stream, d_rd, (const uint32_t *)c->g.d_deg.get(), n, w.d_tids.get(), w.d_tkey.get(), tcap);
        ev.begin(EV_SW_SORT);
        if (!tiles.empty()) hipLaunchKernelGGL(k_sweep_sort_lds, dim3((unsigned)tiles.size()), dim3(BLOCK), 0, c->stream, w.d_tids.get(), w.d_tkey.get(), tcap, d_tiles, T, 0u);
        if (!grows.empty())
            for (uint64_t k = 2 * (uint64_t)T; k <= maxP; k *= 2) {
                for (uint64_t j = k / 2; j >= T; j /= 2)
                    hipLaunchKernelGGL(k_sweep_sort_step, dim3(gx(maxP / 2), (unsigned)grows.size()), dim3(BLOCK), 0, c->stream, w.d_tids.get(), w.d_tkey.get(), tcap,
                                       d_grows, (uint32_t)k, (uint32_t)j);
                if (T >= 2) hipLaunchKernelGGL(k_sweep_sort_lds, dim3((unsigned)tiles.size()), dim3(BLOCK), 0, c->stream, w.d_tids.get(), w.d_tkey.get(), tcap, d_tiles, T, (uint32_t)k);
            }
        ev.end();
    }
    // rank maps, cut counts, scans: rank_rows rows at a time
    ev.begin(EV_SW_CUT);
    w.rank_dirty = true;
    for (int r0 = 0; r0 < nb; r0 += (int)w.rank_rows) {
        const unsigned nr = (unsigned)std::min<int>((int)w.rank_rows, nb - r0);
        if (maxL) {
            hipLaunchKernelGGL(k_sweep_scatter<true>, dim3(gx(maxL), nr), dim3(BLOCK), 0, c->stream, d_rd, (uint32_t)r0, w.d_rank.get(), n, (const int32_t *)w.d_tids.get(), tcap,
                               (const uint32_t *)c->g.d_deg.get(), w.d_ids.get(), w.d_cut.get(), w.d_vol.get(), hcap);
            hipLaunchKernelGGL(k_sweep_cut, dim3(gx(maxL), nr), dim3(BLOCK), 0, c->stream, d_rd, (uint32_t)r0, (const int32_t *)w.d_rank.get(), n, (const int64_t *)c->g.d_row_ptr.get(),
                               (const int32_t *)c->g.d_col.get(), (const int32_t *)w.d_ids.get(), (unsigned long long *)w.d_cut.get(), hcap);
        }
        hipLaunchKernelGGL(k_sweep_scan, dim3(nr), dim3(BLOCK), 0, c->stream, d_rd, (uint32_t)r0, w.d_cut.get(), w.d_vol.get(), hcap, (uint64_t)c->g.nnz, w.d_out.get());
        if (maxL)
            hipLaunchKernelGGL(k_sweep_scatter<false>, dim3(gx(maxL), nr), dim3(BLOCK), 0, c->stream, d_rd, (uint32_t)r0, w.d_rank.get(), n, (const int32_t *)w.d_tids.get(), tcap,
                               (const uint32_t *)nullptr, (int32_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0);
    }
    ev.end();
    HIPCHK(c, hipMemcpyAsync(w.h_out.get(), w.d_out.get(), (size_t)nb * sizeof(SweepRowOut), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, FORA_E_HIP, std::string("sweep: ") + hipGetErrorString(e));
    w.rank_dirty = false;
    for (int i = 0; i < nb; i++) {
        const SweepRowOut &o = w.h_out.get()[i];
        sw.rows[(size_t)row_of(i)] = sweep_row_of(o.len, o.best, o.cut, o.vol, o.den);
        sw.edges += o.edges;
    }
    return FORA_OK;
}

int sweep_finish(fora_ctx *c, SweepRun &sw, int64_t *row_ptr, fora_sweep_row *rows, fora_sweep_stats *out) {
    SweepResult &w = c->swp;
    sw.lay.finish();
    if (int rc = sweep_reserve(c, sw.lay)) return rc; // (only grows when dangling rows came last)
    if (int rc = finish_rows(c, sw.lay, w, "sweep result", row_ptr, [&](uint32_t nd, const int64_t *at, const int32_t *src) {
            hipLaunchKernelGGL(k_sweep_single, dim3((nd + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, nd, at, src,
                               w.d_ids.get(), w.d_cut.get(), w.d_vol.get(), (uint64_t)w.d_ids.size());
        })) return rc;
    if (rows && sw.lay.nq) memcpy(rows, sw.rows.data(), (size_t)sw.lay.nq * sizeof(fora_sweep_row));
    if (out) {
        memset(out, 0, sizeof(*out));
        out->entries = sw.lay.support; out->max_row = sw.lay.max_row; out->thr_fix = sw.thr; out->edges = sw.edges;
        out->batches = sw.lay.batches; out->global_rows = sw.global_rows;
        out->compact_ms = c->tm.sw_compact_ms; out->sort_ms = c->tm.sw_sort_ms; out->cut_ms = c->tm.sw_cut_ms;
    }
    return FORA_OK;
}

// refinement launches after k_walk_alloc: indexed walks, online walks, and the accumulate of their results
// k_walk_dg as the launch selects it: the instantiation, and the bytes of its tables in dynamic LDS (fora_tables.h)
typedef void (*WalkDgKernel)(Dev, uint32_t);
// the option "walk_flush_align" as the kernels know it: results per aligned line of a flush, 0 / 8 / 16
static int walk_flush_align(const fora_ctx *c) { const int64_t v = c->opt_.walk_flush_align; return v >= 16 ? 16 : v >= 8 ? 8 : 0; }
template <int G>
static WalkDgKernel walk_dg_arm(int which) {
    switch (which) {
    case 0: return k_flush_arm_walk_dg<G, false, false, false>;
    case 1: return k_flush_arm_walk_dg<G, false, false, true>;
    case 2: return k_flush_arm_walk_dg<G, false, true, false>;
    case 3: return k_flush_arm_walk_dg<G, false, true, true>;
    case 4: return k_flush_arm_walk_dg<G, true, false, false>;
    case 5: return k_flush_arm_walk_dg<G, true, false, true>;
    case 6: return k_flush_arm_walk_dg<G, true, true, false>;
    default: return k_flush_arm_walk_dg<G, true, true, true>;
    }
}
static WalkDgKernel walk_dg_kernel(bool nzh, bool bits32, bool xl, int align) {
    const int which = (nzh ? 4 : 0) | (bits32 ? 2 : 0) | (xl ? 1 : 0);
    if (align != DG_FLUSH_ALIGN) { // the other arms of the flush (every arm has the default's LDS and launch shape)
        if constexpr (DG_FLUSH_ALIGN != 0) if (align == 0) return walk_dg_arm<0>(which);
        if constexpr (DG_FLUSH_ALIGN != 8) if (align == 8) return walk_dg_arm<8>(which);
        if constexpr (DG_FLUSH_ALIGN != 16) if (align == 16) return walk_dg_arm<16>(which);
    }
    switch (which) {
    case 0: return k_walk_dg<false, false, false>;
    case 1: return k_walk_dg<false, false, true>;
    case 2: return k_walk_dg<false, true, false>;
    case 3: return k_walk_dg<false, true, true>;
    case 4: return k_walk_dg<true, false, false>;
    case 5: return k_walk_dg<true, false, true>;
    case 6: return k_walk_dg<true, true, false>;
    default: return k_walk_dg<true, true, true>;
    }
}
static size_t walk_dg_lds(const WalkDG &g, bool xl) { return walk_dg_lds_bytes(g.H, g.nrec, g.nblk, xl); }

void launch_walks(fora_ctx *c, const Dev &d, int nq, bool with_idx, uint32_t round, int nzh) {
    const WsPlan &p = c->ws.plan;
    const dim3 wg(walk_grid_x(c, nq), nq);
    const dim3 wgs(p.binned ? p.sub : 1u, nq); // kernels that fill buckets: one workgroup per sub-bucket (Dev::bk_w)
    EvSpan ev(c, EV_WALK);
    if (with_idx) {
        if (!p.binned) hipLaunchKernelGGL(k_walk_idx<1>, wg, dim3(BLOCK), 0, c->stream, d);
        else if (!d.wide) hipLaunchKernelGGL(k_walk_idx<MAX_BINS>, wgs, dim3(BLOCK), 0, c->stream, d);
        else
            for (int lo = 0; lo < p.nbins; lo += p.pbins) { // buckets are reused pass by pass
                Dev dp = d;
                dp.bin_lo = lo;
                dp.bin_cnt = std::min(p.pbins, p.nbins - lo);
                const dim3 wgi = (dp.slot_major & 4u) ? dim3(wgs.y, wgs.x) : wgs;
                if (p.pbins > MAX_BINS_WIDE) hipLaunchKernelGGL(k_walk_idx<MAX_BINS_HUGE>, wgi, dim3(BIN_THREADS_HUGE), 0, c->stream, dp);
                else hipLaunchKernelGGL(k_walk_idx<MAX_BINS_WIDE>, wgi, dim3(BIN_THREADS_WIDE), 0, c->stream, dp);
                { const unsigned gx = acc_grid(c, dp, nq); hipLaunchKernelGGL((k_accum<true, true>), (dp.slot_major & 2u) ? dim3(nq, gx) : dim3(gx, nq), dim3(ACC_THREADS_WIDE), 0, c->stream, dp, 0); }
            }
    }
    const bool dg = p.binned && !d.wide && d.dg.colp && c->opt_.walk_dg != 0; // narrow layout: one gather per step over the degree-grouped copy
    const bool xl = dg && c->opt_.walk_dg != 1 && d.dg.invb;                  // ... and results in bucket order (no gather per walk either)
    if (xl && with_idx) { // the indexed results are in plain ids: reduce them before the buckets are reused in bucket order
        ev.begin(EV_WALK_ACCUM);
        hipLaunchKernelGGL((k_accum<true, false>), dim3(p.nbins, nq), dim3(ACC_THREADS), 0, c->stream, d, 0);
        ev.begin(EV_WALK);
    }
    Dev dw = d;
    if (xl) { dw.nbins = (int32_t)d.dg.nbx; dw.acc_xl = d.dg.invb; }
    if (dg) {
        hipLaunchKernelGGL(walk_dg_kernel(nzh != 0, d.dg.bits32 != 0, xl, walk_flush_align(c)), wgs, dim3(DG_THREADS), walk_dg_lds(d.dg, xl), c->stream, dw, round);
    } else
        hipLaunchKernelGGL(k_walk_online<WALK_TO_PPR>, p.binned && !d.wide ? wgs : wg, dim3(BLOCK), 0, c->stream, d, round, nzh, (int32_t *)nullptr);
    ev.end();
    if (p.binned && !d.wide) { // narrow layout: indexed and online results share the buckets (bucket-order results: see above)
        ev.begin(EV_WALK_ACCUM);
        hipLaunchKernelGGL((k_accum<true, false>), dim3(dw.nbins, nq), dim3(ACC_THREADS), 0, c->stream, dw, 0);
    }
}

static hipError_t ensure_active(Workspace &w) { return w.d_active.ensure((size_t)w.B); } // marks of the slots that run a round: --balanced and the top-k drivers
// --balanced push of a batch (query.h:848-884): rounds of the incremental push (algo.h:1020-1093) with rmax halving
// from 8*config.rmax; a slot keeps going while its estimated walk cost exceeds what its push has cost so far.
int push_balanced(fora_ctx *c, const int32_t *sources, int nq, bool with_idx) {
    HIPCHK(c, ensure_active(c->ws));
    const uint32_t chunks = slab_grid_x(c, std::min(nq, c->ws.B));
    Dev d = make_dev(c, nq, with_idx);
    EvSpan ev(c, EV_OTHER);
    hipLaunchKernelGGL(k_init_batch, dim3((nq + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, d, 1);
    ev.end();
    std::vector<uint8_t> active((size_t)nq, 1);
    std::vector<uint64_t> rsum_fix((size_t)nq, FIX_ONE), pops((size_t)nq, 0), relax((size_t)nq, 0);
    c->bal.h_rmax_used.assign((size_t)nq, c->par.rmax);
    c->bal.h_rounds.assign((size_t)nq, 1);
    for (int i = 0; i < nq; i++)
        if (is_dangling(c, sources[i])) active[i] = 0; // :864, :882
    for (int i = 0; i < nq; i++) if (active[i]) c->bal.h_rounds[i] = 0;
    double rmax = c->par.rmax * c->bal.start; // :862
    for (int round = 0;; round++) {
        bool any = false;
        for (int i = 0; i < nq; i++) {
            if (!active[i]) continue;
            const double t = (!with_idx || rmax >= c->par.rmax) ? c->bal.t_walk : c->bal.t_idx;                       // :825-838
            const double est = c->par.omega * std::ldexp((double)rsum_fix[i], -62) * (1 - c->par.alpha) * t;
            const double used = (double)pops[i] * c->bal.c_pop + (double)relax[i] * c->bal.c_edge;
            if (!(est > used)) active[i] = 0;                                                              // :866
            else { any = true; c->bal.h_rmax_used[i] = rmax; c->bal.h_rounds[i] = round + 1; }
        }
        if (!any) break;
        if (round >= 64) return fail(c, FORA_E_OVERFLOW, "--balanced: rmax halved 64 times");
        HIPCHK(c, hipMemcpyAsync(c->ws.d_active.get(), active.data(), (size_t)nq, hipMemcpyHostToDevice, c->stream));
        if (round) {
            HIPCHK(c, c->ws.d_counters.zero(c->stream));
            int rc = reset_binned_counters(c);
            if (rc) return rc;
        }
        Dev dr = make_dev(c, nq, with_idx, rmax, c->par.omega);
        ev.begin(EV_OTHER);
        hipLaunchKernelGGL(k_topk_frontier, dim3(chunks, nq), dim3(BLOCK), 0, c->stream, dr, (const uint8_t *)c->ws.d_active.get());
        ev.end();
        int rc = run_push_levels(c, dr, nullptr, 0, true);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(c->h_qs.data(), c->ws.d_qs.get(), (size_t)nq * sizeof(QState), hipMemcpyDeviceToHost));
        for (int i = 0; i < nq; i++) {
            rsum_fix[i] = FIX_ONE - c->h_qs[i].reserved;
            pops[i] = c->h_qs[i].pops;
            relax[i] = c->h_qs[i].relax;
        }
        rmax /= 2; // :875
    }
    return FORA_OK;
}

// One batch of <= B sources: push (+ refinement) and k_ppr_sum, then the batch's close-out; its per-slot accumulators
// land in h_qs.  Results stay in the slabs.
int run_query_batch(fora_ctx *c, const int32_t *sources, int nq, bool with_idx, int flags, const SparseRun *sp = nullptr) {
    EvSpan batch(c, EV_BATCH);
    int rc = reset_batch_state(c, nq, sources);
    if (rc) return rc;
    Dev d = make_dev(c, nq, with_idx);
    EvSpan ev(c);
    if (c->bal.on) {
        rc = push_balanced(c, sources, nq, with_idx);
    } else {
        if (TEST_PATHS && c->ws.plan.binned) d.rounds = (int32_t)std::min<int64_t>(std::max<int64_t>(c->opt_.rounds, 1), 16);
        d.round_div = (uint32_t)std::min<int64_t>(std::max<int64_t>(c->opt_.round_div, 0), 1 << 20);
        const bool team = use_team(c, d);
        ev.begin(EV_OTHER);
        hipLaunchKernelGGL(k_init_batch, dim3((nq + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, d, team ? 3 : 0);
        ev.end();
        rc = team ? run_push_team(c, d) : run_push_levels(c, d);
        d.rounds = 1;
    }
    if (rc) return rc;
    if (!(flags & RUN_PUSH_ONLY)) {
        const uint32_t chunks = slab_grid_x(c, nq);
        ev.begin(EV_WALK_ALLOC);
        hipLaunchKernelGGL(k_walk_alloc<ALLOC_QUERY>, (d.wide && (d.slot_major & 8u)) ? dim3(nq, chunks) : dim3(chunks, nq), dim3(BLOCK), 0, c->stream, d, with_idx ? 1 : 0,
                           (const uint8_t *)nullptr, (uint64_t *)nullptr, (unsigned long long *)nullptr, 0u);
        ev.end();
        launch_walks(c, d, nq, with_idx, 0u, c->par.opt ? 1 : 0);
    }
    {
        const uint32_t chunks = (uint32_t)std::min<int64_t>(((int64_t)c->g.n + BLOCK - 1) / BLOCK, 64);
        ev.begin(EV_OTHER);
        hipLaunchKernelGGL(k_ppr_sum, dim3(chunks, nq), dim3(BLOCK), 0, c->stream, d);
        ev.end();
    }
    if (sp) if ((rc = count_rows(c, *sp, nullptr, nq, c->sp.cnt, EV_SP_COMPACT))) return rc; // (inside the batch: the counts come back with its close-out)
    HIPCHK(c, hipMemcpyAsync(c->ws.h_qs_pin.get(), c->ws.d_qs.get(), (size_t)nq * sizeof(QState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ws.h_steps_pin.get(), d.tot_steps, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if ((rc = close_batch(c, &batch, "batch"))) return rc;
    for (int i = 0; i < nq; i++) c->h_qs[i] = c->ws.h_qs_pin.get()[i];
    c->tm.total.walk_steps += *c->ws.h_steps_pin.get();
    fold_counters(c, c->h_qs.data(), nq);
    return FORA_OK;
}

// stats of slot i of the batch just run
void fill_stats(const fora_ctx *c, int i, fora_query_stats &o) {
    const QState &s = c->h_qs[i];
    o.rsum_fix = FIX_ONE - s.reserved;
    o.rsum = std::ldexp((double)o.rsum_fix, -62);
    o.n_rw = s.n_rw; o.n_walks = s.n_walks; o.n_idx_hit = s.n_hit;
    o.pops = s.pops; o.relax = s.relax; o.ppr_sum_fix = s.ppr_sum;
    o.levels = (int32_t)s.levels; o.dangling_source = (int32_t)s.dangling_source;
    o.rmax_used = c->bal.on && (size_t)i < c->bal.h_rmax_used.size() ? c->bal.h_rmax_used[i] : c->par.rmax;
    o.push_rounds = c->bal.on && (size_t)i < c->bal.h_rounds.size() ? c->bal.h_rounds[i] : 1;
    o.reserved_ = 0;
}

// workspace of a call of `slots` queries at the ctx's omega, and the (ids, scores) pair of k entries per slot when k > 0
int ensure_query_workspace(fora_ctx *c, int slots, int k) {
    c->retry.div = 1; // (queries with smaller buckets, measured: LJ-sized 350 -> 220 q/s -- the indexed walks' results overflow into direct atomics; Twitter-2010-sized: no change)
    if (int rc = ensure_workspace(c, slots, c->par.omega)) return rc;
    return k > 0 ? grow_pair(c, k, c->ws.d_topk_ids, c->ws.d_topk_sc) : FORA_OK;
}

// topk > 0: also the top-k of each slot's ppr slab (k_topk_select: score descending, ties id ascending, padded with (0, 0.0))
// into ids / scores (either may be null); the caller has checked 1 <= topk <= min(SEL_MAXK, n).
int query_common(fora_ctx *c, const int32_t *sources, int nq, int with_idx, int flags, double *ppr_d,
                 uint64_t *ppr_fix, uint64_t *residue_fix, fora_query_stats *stats, int topk = 0, int32_t *ids = nullptr,
                 double *scores = nullptr, SparseRun *sp = nullptr, SweepRun *sw = nullptr) {
    if (int rc = check_batch_args(c, sources, nq)) return rc;
    if (with_idx && !c->ix.have) return fail(c, FORA_E_ARG, "with_idx without an index (build or set one)");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = check_id_range(c, sources, nq)) return rc;
    const uint64_t n = (uint64_t)c->g.n;
    // A dangling source is its own whole answer (algo.h:961-965: reserve[s] = 1, rsum = 0, no push, no walks): it is
    // written here and never takes a slot.  (On the R-MAT variant with 52 % dangling nodes half of a batch's slots were
    // such sources, and every level launch and the tail kernel carried their empty workgroups: push of 1000 queries
    // 66.5 ms against 38 for the 483 others alone.)
    std::vector<int32_t> live_src;
    std::vector<int> live_at; // position of live source i in the caller's arrays
    for (int i = 0; i < nq; i++) {
        const int32_t s = sources[i];
        if (!is_dangling(c, s)) { live_src.push_back(s); live_at.push_back(i); continue; }
        if (stats) {
            fora_query_stats &o = stats[i];
            memset(&o, 0, sizeof(o));
            o.ppr_sum_fix = FIX_ONE; o.dangling_source = 1; o.rmax_used = c->par.rmax; o.push_rounds = 1;
        }
        if (ppr_d) { double *row = ppr_d + (uint64_t)i * n; memset(row, 0, n * 8); row[s] = 1.0; }
        if (ppr_fix) { uint64_t *row = ppr_fix + (uint64_t)i * n; memset(row, 0, n * 8); row[s] = FIX_ONE; }
        if (residue_fix) memset(residue_fix + (uint64_t)i * n, 0, n * 8);
        if (topk > 0) { // one non-zero entry, then the padding
            if (ids) { int32_t *row = ids + (uint64_t)i * topk; memset(row, 0, (size_t)topk * 4); row[0] = s; }
            if (scores) { double *row = scores + (uint64_t)i * topk; memset(row, 0, (size_t)topk * 8); row[0] = 1.0; }
        }
    }
    const bool want_topk = topk > 0 && (ids || scores);
    const int nl = (int)live_src.size();
    if (sp) sp->lay.begin(sources, nq);
    if (sw) sw->lay.begin(sources, nq);
    if (nl == 0) return FORA_OK;
    int rc = FORA_OK;
    if (sw) if ((rc = sweep_prepare_rank(c, nl))) return rc; // (ahead of the workspace: a batch size chosen from the free memory accounts for the block)
    rc = ensure_query_workspace(c, nl, want_topk ? topk : 0);
    if (rc) return rc;
    const int per = even_batch(nl, c->ws.B);
    if (sw) if ((rc = sweep_prepare(c, *sw, std::min(per, nl)))) return rc;
    if (sp) if ((rc = sparse_prepare(c, *sp, std::min(per, nl), nl))) return rc;
    for (int b0 = 0; b0 < nl; b0 += per) {
        const int nb = std::min(per, nl - b0);
        const int *at = live_at.data() + b0; // places of the batch's slots in the caller's arrays
        if ((rc = run_query_batch(c, live_src.data() + b0, nb, with_idx != 0, flags, sp))) return rc;
        if (stats) for (int i = 0; i < nb; i++) fill_stats(c, i, stats[at[i]]);
        if (sp) if ((rc = sparse_place(c, *sp, at, 0, nb))) return rc;
        if (sw) if ((rc = sweep_rows_of_batch(c, *sw, at, 0, nb))) return rc;
        if (want_topk) {
            if ((rc = launch_select(c, make_dev(c, nb, false), nb, topk, c->ws.d_topk_ids.get(), c->ws.d_topk_sc.get(), 0))) return rc;
            if ((rc = copy_topk_out(c, nb, topk, ids, scores, 0, at))) return rc;
        }
        // slots i .. j - 1 of the batch whose places in the caller's arrays are consecutive too: one copy
        for (int i = 0, j; i < nb && (ppr_d || ppr_fix || residue_fix); i = j) {
            for (j = i + 1; j < nb && at[j] == at[j - 1] + 1; j++) {}
            if ((rc = copy_slab_out(c, c->ws.d_ppr.get(), i, at[i], j - i, ppr_fix, ppr_d, 62))) return rc;
            if ((rc = copy_slab_out(c, c->ws.d_residue.get(), i, at[i], j - i, residue_fix, nullptr, 62))) return rc;
        }
    }
    return FORA_OK;
}

// ---- seed sets (fora_hip_query_seeds_batch; the SEED SETS contract of include/fora_hip.h).  PPR is linear in the restart
// vector: every seed a call needs runs once as an ordinary query (run_query_batch), and k_seed_combine folds the batch's ppr
// slabs into one accumulator row per set before the next batch reuses them.  Nothing of the push or the walks knows of sets.
// The planning of a call -- checks, weights, slots, batches and the words of the uploads -- is fora_seeds_plan.h.

// the combine of the batch just closed: its slabs hold the rows until the next batch starts on the same stream
int seed_combine(fora_ctx *c, const SeedBatch &b) {
    if (!b.U) return FORA_OK;
    HIPCHK(c, hipMemcpyAsync(c->sd.d_list.get(), b.pack.data(), b.pack.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (pageable source)
    const SeedListView<const uint64_t> l = b.list(c->sd.d_list.get());
    const uint32_t n = (uint32_t)c->g.n;
    const CompactGeom geo = seed_combine_geom(n);
    EvSpan ev(c, EV_SEED_COMBINE);
    for (uint32_t y0 = 0; y0 < b.T; y0 += 65535)
        hipLaunchKernelGGL(k_seed_combine, dim3(geo.X, std::min<uint32_t>(65535, b.T - y0)), dim3(BLOCK), 0, c->stream, (const uint64_t *)c->ws.d_ppr.get(), n, geo.R,
                           l.set_id() + y0, l.seg() + y0, l.use_slot(), l.use_w(), c->sd.d_acc.get());
    return FORA_OK;
}

// What the three entry points over seed sets share: the arguments checked, the weights at 2^-62, the slots, the accumulator
// block, the batches with their combines and the dangling seeds' terms.  It leaves the finished block acc[ns][n] (c->sd.d_acc)
// on the stream -- a set row is complete only here, after the last batch -- and the counts of *st in sc.  ns == 0: FORA_OK and
// nothing done.  k: of a top-k the caller will take from the workspace's select (0: none); sweep: the sweep's rank block is
// wanted too (after the accumulator block and ahead of the workspace, so that a batch size chosen from the free memory
// accounts for both).
struct SeedCounts { uint64_t seeds = 0, distinct = 0, queries = 0, dangling = 0; int batches = 0; };
int seeds_accumulate(fora_ctx *c, const int64_t *set_ptr, const int32_t *seeds, const double *weights, int ns, int with_idx,
                     int k, bool want_topk, bool sweep, fora_seeds_stats *st, SeedCounts &sc) {
    if (int rc = check_batch_args(c, nullptr, 0)) return rc;
    const char *bad = seed_sets_error(set_ptr, seeds, ns);
    if (st && ns >= 0) memset(st, 0, sizeof(*st)); // (a negative count leaves *st as it was)
    if (bad) return fail(c, FORA_E_ARG, bad);
    if (ns == 0) return FORA_OK;
    const int64_t total = set_ptr[ns];
    if (with_idx && !c->ix.have) return fail(c, FORA_E_ARG, "with_idx without an index (build or set one)");
    if (k != 0) if (int rc = check_k(c, k)) return rc; // (0: no top-k)
    if (int rc = check_id_range(c, seeds, (int)total, "seed")) return rc;
    std::vector<uint64_t> wfix;
    if ((bad = seed_weights(set_ptr, weights, ns, wfix))) return fail(c, FORA_E_ARG, bad);
    HIPCHK(c, hipSetDevice(c->device));
    c->tm.seed_combine_ms = 0;
    const uint64_t n = (uint64_t)c->g.n;
    const SeedSlots slots = seed_slots(set_ptr, seeds, wfix.data(), ns, c->g.h_row_ptr.data(), c->opt_.seeds_dedup != 0);
    const int nl = (int)slots.slot_src.size();
    // The accumulator block, ahead of the workspace: a batch size chosen from the free memory then accounts for it.  No room
    // beside a workspace that is already there: that one goes, and the call plans a new one in what the block leaves.
    const uint64_t cells = (uint64_t)ns * n;
    const char *const no_room = "no device memory for the seed sets' accumulator block (ns x n words): split the call";
    if (cells > (1ull << 40)) return fail(c, FORA_E_NOMEM, no_room); // (8 TB: more than any device holds, and cells * 8 stays far from 2^64)
    if (c->sd.d_acc.ensure(cells) != hipSuccess) {
        (void)hipGetLastError();
        free_workspace(c);
        if (c->sd.d_acc.ensure(cells) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, FORA_E_NOMEM, no_room);
        }
    }
    HIPCHK(c, c->sd.d_acc.zero(c->stream, cells));
    int rc = FORA_OK;
    int nbatch = 0;
    if (sweep) if ((rc = sweep_prepare_rank(c, ns))) return rc;
    if (nl > 0 || want_topk) {
        if ((rc = ensure_query_workspace(c, std::max(nl, 1), want_topk ? k : 0))) return rc;
    }
    if (nl > 0) {
        const int per = even_batch(nl, c->ws.B);
        nbatch = (nl + per - 1) / per;
        const std::vector<SeedBatch> batches = seed_batches(slots.uses, nl, per);
        size_t words = 0;
        for (const SeedBatch &b : batches) words = std::max(words, b.pack.size());
        HIPCHK(c, c->sd.d_list.ensure(std::max<size_t>(words, 1)));
        for (int bi = 0; bi < nbatch; bi++) {
            const int b0 = bi * per, nb = std::min(per, nl - b0);
            if ((rc = run_query_batch(c, slots.slot_src.data() + b0, nb, with_idx != 0, 0))) return rc;
            if ((rc = seed_combine(c, batches[(size_t)bi]))) return rc;
        }
    }
    const size_t nd = slots.dang_set.size();
    if (nd) {
        const std::vector<uint64_t> pack = seed_dangling_pack(slots);
        HIPCHK(c, hipStreamSynchronize(c->stream)); // (the last combine reads the list)
        HIPCHK(c, c->sd.d_list.ensure(pack.size()));
        HIPCHK(c, hipMemcpyAsync(c->sd.d_list.get(), pack.data(), pack.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); // (pageable source)
        const SeedDanglingView<const uint64_t> d{c->sd.d_list.get(), nd};
        hipLaunchKernelGGL(k_seed_single, dim3((unsigned)((nd + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, (uint32_t)nd, d.set(), d.node(), d.w(), (uint32_t)n,
                           c->sd.d_acc.get());
    }
    sc.seeds = (uint64_t)total; sc.distinct = slots.distinct; sc.queries = (uint64_t)nl; sc.dangling = (uint64_t)nd; sc.batches = nbatch;
    return FORA_OK;
}

// the sums over the whole rows of the finished block, on their way to the caller's array (the stream is not synchronised)
int seed_row_sums(fora_ctx *c, int ns, uint64_t *row_sum_fix_out) {
    const uint64_t n = (uint64_t)c->g.n;
    HIPCHK(c, c->sd.d_sums.ensure((size_t)ns));
    HIPCHK(c, c->sd.d_sums.zero(c->stream, (size_t)ns));
    const unsigned chunks = (unsigned)std::min<uint64_t>((n + BLOCK - 1) / BLOCK, 64);
    hipLaunchKernelGGL(k_seed_row_sum, dim3((unsigned)ns, chunks), dim3(BLOCK), 0, c->stream, (const uint64_t *)c->sd.d_acc.get(), (uint32_t)n, c->sd.d_sums.get());
    HIPCHK(c, hipMemcpyAsync(row_sum_fix_out, c->sd.d_sums.get(), (size_t)ns * 8, hipMemcpyDeviceToHost, c->stream));
    return FORA_OK;
}

void fill_seeds_stats(const fora_ctx *c, const SeedCounts &sc, fora_seeds_stats *st) { // (after ev_collect)
    if (!st) return;
    st->seeds = sc.seeds; st->distinct = sc.distinct; st->queries = sc.queries; st->dangling = sc.dangling;
    st->batches = sc.batches; st->combine_ms = c->tm.seed_combine_ms;
}

// fora_hip_query_seeds_batch: the output stage over the finished block
int query_seeds_impl(fora_ctx *c, const int64_t *set_ptr, const int32_t *seeds, const double *weights, int ns, int with_idx,
                     double *ppr_out, uint64_t *ppr_fix_out, int k, int32_t *ids, double *scores, uint64_t *row_sum_fix_out,
                     fora_seeds_stats *st) {
    const bool want_topk = k > 0 && (ids || scores);
    SeedCounts sc;
    int rc = seeds_accumulate(c, set_ptr, seeds, weights, ns, with_idx, k, want_topk, false, st, sc);
    if (rc || ns == 0) return rc;
    const uint64_t n = (uint64_t)c->g.n, cells = (uint64_t)ns * n;
    uint64_t *const acc = c->sd.d_acc.get();
    if (row_sum_fix_out) if ((rc = seed_row_sums(c, ns, row_sum_fix_out))) return rc;
    if (want_topk)
        for (int r0 = 0; r0 < ns; r0 += c->ws.B) { // the select works on the slots of a workspace: at most B rows at a time
            const int nb = std::min(c->ws.B, ns - r0);
            Dev ds = make_dev(c, nb, false);
            ds.ppr = acc + (uint64_t)r0 * n;
            if ((rc = launch_select(c, ds, nb, k, c->ws.d_topk_ids.get(), c->ws.d_topk_sc.get(), 0))) return rc;
            if ((rc = copy_topk_out(c, nb, k, ids, scores, (uint64_t)r0))) return rc;
        }
    if (ppr_fix_out) HIPCHK(c, hipMemcpyAsync(ppr_fix_out, acc, cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (ppr_out) { // in place: the block has no reader left
        hipLaunchKernelGGL(k_seed_f64, dim3((unsigned)std::min<uint64_t>((cells + BLOCK - 1) / BLOCK, 8192)), dim3(BLOCK), 0, c->stream, acc, cells);
        HIPCHK(c, hipMemcpyAsync(ppr_out, acc, cells * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, FORA_E_HIP, std::string("seed sets: ") + hipGetErrorString(e));
    ev_collect(c);
    fill_seeds_stats(c, sc, st);
    return FORA_OK;
}

// rows of the finished block that fora_hip_seeds_sparse_batch / fora_hip_seeds_sweep_batch compact (and sort) at a time
int seeds_chunk(const fora_ctx *c) { return fora::seeds_chunk(c->opt_.seeds_rows, (uint64_t)c->g.n); }

// one attempt of fora_hip_seeds_sparse_batch: the block, then count / place over its rows, every row live and no dangling one
int seeds_sparse_impl(fora_ctx *c, const int64_t *set_ptr, const int32_t *seeds, const double *weights, int ns, int with_idx,
                      uint64_t thr, int64_t *row_ptr, uint64_t *row_sum_fix_out, fora_seeds_stats *st, fora_sparse_stats *sp_out,
                      int64_t topk = 0, fora_topk_stats *tk_out = nullptr) {
    SparseRun run; // (a retried attempt starts from an empty one)
    run.thr = thr; run.topk = topk;
    c->tm.sp_compact_ms = c->tm.tk_select_ms = 0;
    if (sp_out) memset(sp_out, 0, sizeof(*sp_out));
    if (tk_out) memset(tk_out, 0, sizeof(*tk_out));
    SeedCounts sc;
    int rc = seeds_accumulate(c, set_ptr, seeds, weights, ns, with_idx, 0, false, false, st, sc);
    if (rc) return rc;
    run.lay.begin(nullptr, ns);
    if (ns == 0) { // an empty result is held; the stats stay zero
        HIPCHK(c, hipSetDevice(c->device));
        return sparse_finish(c, run, row_ptr, nullptr);
    }
    const uint64_t n = (uint64_t)c->g.n;
    const int C = seeds_chunk(c);
    if ((rc = sparse_prepare(c, run, std::min(C, ns), ns))) return rc;
    for (int r0 = 0; r0 < ns; r0 += C) {
        const int nb = std::min(C, ns - r0);
        const uint64_t *rows = c->sd.d_acc.get() + (uint64_t)r0 * n;
        if ((rc = count_rows(c, run, rows, nb, c->sp.cnt, EV_SP_COMPACT))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream)); // (the counts are back)
        if ((rc = sparse_place(c, run, nullptr, r0, nb, rows))) return rc;
    }
    if (row_sum_fix_out) if ((rc = seed_row_sums(c, ns, row_sum_fix_out))) return rc;
    if ((rc = sparse_finish(c, run, row_ptr, sp_out, tk_out))) return rc;
    fill_seeds_stats(c, sc, st);
    return FORA_OK;
}

// one attempt of fora_hip_seeds_sweep_batch: the block, then the sweep's passes over its rows
int seeds_sweep_impl(fora_ctx *c, const int64_t *set_ptr, const int32_t *seeds, const double *weights, int ns, int with_idx,
                     uint64_t thr, int64_t max_size, int64_t *row_ptr, fora_sweep_row *rows_out, fora_seeds_stats *st, fora_sweep_stats *sw_out) {
    SweepRun run(thr, max_size, ns); // (a retried attempt starts from an empty one)
    c->tm.sw_compact_ms = c->tm.sw_sort_ms = c->tm.sw_cut_ms = 0;
    if (sw_out) memset(sw_out, 0, sizeof(*sw_out));
    SeedCounts sc;
    int rc = seeds_accumulate(c, set_ptr, seeds, weights, ns, with_idx, 0, false, true, st, sc);
    if (rc) return rc;
    run.lay.begin(nullptr, ns);
    if (ns == 0) { // an empty result is held; the stats stay zero
        HIPCHK(c, hipSetDevice(c->device));
        return sweep_finish(c, run, row_ptr, rows_out, nullptr);
    }
    const uint64_t n = (uint64_t)c->g.n;
    const int C = seeds_chunk(c);
    if ((rc = sweep_prepare(c, run, std::min(C, ns)))) return rc;
    for (int r0 = 0; r0 < ns; r0 += C) {
        const int nb = std::min(C, ns - r0);
        if ((rc = sweep_rows_of_batch(c, run, nullptr, r0, nb, c->sd.d_acc.get() + (uint64_t)r0 * n))) return rc;
    }
    if ((rc = sweep_finish(c, run, row_ptr, rows_out, sw_out))) return rc;
    fill_seeds_stats(c, sc, st);
    return FORA_OK;
}

// ---- frame of the two top-k drivers (fora_hip_topk_batch, fora_hip_topk_bound_batch): all active slots of a batch are
// in the same round, so delta / rmax / omega are uniform per round; finished slots drop out.  Each driver keeps its own
// delta schedule, rmax / omega formulas, bounds kernels and stop rule.

// The index cursors of a new batch all read as zero: a new epoch (the slabs themselves are cleared when they are allocated
// and when the 24-bit epoch wraps).
int next_cursor_epoch(fora_ctx *c) {
    if (c->ws.cursor_epoch == 0 || c->ws.cursor_epoch >= 0xFFFFFFu) {
        HIPCHK(c, c->ws.d_cursor.zero(c->stream));
        c->ws.cursor_epoch = 0;
    }
    c->ws.cursor_epoch++;
    return FORA_OK;
}

// slabs of the drivers: ppr2 (the rounds' ppr), index cursors, active marks, per-slot counts; the (ids, scores) pair
int ensure_topk_slabs(fora_ctx *c, int k) {
    Workspace &w = c->ws;
    const uint64_t slab = (uint64_t)w.B * (uint64_t)c->g.n;
    HIPCHK(c, w.d_ppr2.ensure(slab));
    if (!w.d_cursor) w.cursor_epoch = 0; // new slabs hold no valid word: next_cursor_epoch clears them
    HIPCHK(c, w.d_cursor.ensure(slab));
    HIPCHK(c, ensure_active(w));
    HIPCHK(c, w.d_above.ensure((size_t)w.B));
    return grow_pair(c, k, w.d_topk_ids, w.d_topk_sc);
}

// host side of a batch; the vectors are kept from batch to batch (asynchronous copies read them)
struct TopkBatch {
    EvSpan span;                      // the batch's event pair (topk_batch_start .. close_batch)
    std::vector<uint8_t> active, inactive;
    std::vector<int32_t> nround;      // rounds each slot has run
};

// Batch start: state reset, a new cursor epoch, k_init_batch.  A dangling source never runs a round (query.h:1007-1011,
// :951-955: one round, ppr = e_s), so its slot starts inactive and its ppr2 := reserve here; every other slot's ppr2 is
// written by its first round's copy (round 5 copied all slots here: one 12-GB slab pass per Twitter-2010-sized batch for nothing).
int topk_batch_start(fora_ctx *c, TopkBatch &tb, const int32_t *sources, int nb, bool with_idx, uint32_t chunks) {
    tb.span.begin(EV_BATCH);
    if (int rc = reset_batch_state(c, nb, sources)) return rc;
    if (with_idx) if (int rc = next_cursor_epoch(c)) return rc; // query.h:997-998, :937-938: every cursor of the batch reads as 0
    hipLaunchKernelGGL(k_init_batch, dim3((nb + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, make_dev(c, nb, with_idx), 1);
    tb.active.assign((size_t)nb, 1);
    tb.inactive.assign((size_t)nb, 0);
    tb.nround.assign((size_t)nb, 1);
    bool any_inactive = false;
    for (int i = 0; i < nb; i++)
        if (is_dangling(c, sources[i])) { tb.active[i] = 0; tb.inactive[i] = 1; any_inactive = true; }
    if (any_inactive) {
        HIPCHK(c, hipMemcpyAsync(c->ws.d_active.get(), tb.inactive.data(), (size_t)nb, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_copy_slab, dim3(chunks, nb), dim3(BLOCK), 0, c->stream, c->g.n, c->ws.d_ppr.get(), c->ws.d_ppr2.get(), (const uint8_t *)c->ws.d_active.get());
    }
    return FORA_OK;
}

// One round of the active slots: the per-round resets, the push from every node at or over the round's threshold
// (algo.h:1020-1093), ppr2 := reserve, then walk allocation (KIND of k_walk_alloc; round_walks: walks per slot, or null) and
// walks into ppr2 (compute_ppr_with_fwdidx_topk, query.h:521-636; ..._with_bound, :639-750).  dw: the round's Dev over ppr2.
template <int KIND>
int topk_round(fora_ctx *c, TopkBatch &tb, int nb, bool with_idx, int round, double rmax, double omega, uint32_t chunks,
               unsigned long long *round_walks, int nzh, Dev &dw) {
    for (int i = 0; i < nb; i++) if (tb.active[i]) tb.nround[i] = round;
    HIPCHK(c, hipMemcpyAsync(c->ws.d_active.get(), tb.active.data(), (size_t)nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, c->ws.d_counters.zero(c->stream));
    HIPCHK(c, c->ws.d_above.zero(c->stream, (size_t)nb));
    HIPCHK(c, c->ws.d_wit_count.zero(c->stream));
    if (int rc = reset_binned_counters(c)) return rc;
    const Dev d = make_dev(c, nb, with_idx, rmax, omega);
    EvSpan ev(c, EV_OTHER);
    hipLaunchKernelGGL(k_topk_frontier, dim3(chunks, nb), dim3(BLOCK), 0, c->stream, d, (const uint8_t *)c->ws.d_active.get());
    ev.end();
    if (int rc = run_push_levels(c, d, nullptr, 0, true)) return rc;
    ev.begin(EV_OTHER);
    hipLaunchKernelGGL(k_copy_slab, dim3(chunks, nb), dim3(BLOCK), 0, c->stream, c->g.n, c->ws.d_ppr.get(), c->ws.d_ppr2.get(),
                       (const uint8_t *)c->ws.d_active.get());
    ev.end();
    dw = d;
    dw.ppr = c->ws.d_ppr2.get();
    ev.begin(EV_WALK_ALLOC);
    hipLaunchKernelGGL(k_walk_alloc<KIND>, (dw.wide && (dw.slot_major & 8u)) ? dim3(nb, chunks) : dim3(chunks, nb), dim3(BLOCK), 0, c->stream, dw, with_idx ? 1 : 0,
                       (const uint8_t *)c->ws.d_active.get(), c->ws.d_cursor.get(), round_walks, c->ws.cursor_epoch);
    ev.end();
    launch_walks(c, dw, nb, with_idx, (uint32_t)round, nzh);
    return FORA_OK;
}

// Batch end: the top k of every slot's ppr2 (topk_ppr, algo.h:592-610; sel_thr: per-slot lower limits of the top k, or
// null), the close-out, ids / scores / rounds of the slots into rows b0 ..., the counters of all their rounds.
int topk_batch_end(fora_ctx *c, TopkBatch &tb, int nb, int k, const double *sel_thr, const char *what, int b0,
                   int32_t *ids, double *scores, int32_t *rounds) {
    Dev ds = make_dev(c, nb, false);
    ds.ppr = c->ws.d_ppr2.get();
    EvSpan ev(c, EV_OTHER);
    if (int rc = launch_select(c, ds, nb, k, c->ws.d_topk_ids.get(), c->ws.d_topk_sc.get(), 0, sel_thr)) return rc;
    ev.end();
    if (int rc = close_batch(c, &tb.span, what)) return rc;
    if (int rc = copy_topk_out(c, nb, k, ids, scores, (uint64_t)b0)) return rc;
    HIPCHK(c, hipMemcpy(c->h_qs.data(), c->ws.d_qs.get(), (size_t)nb * sizeof(QState), hipMemcpyDeviceToHost));
    fold_counters(c, c->h_qs.data(), nb);
    if (rounds) for (int i = 0; i < nb; i++) rounds[b0 + i] = tb.nround[i];
    return FORA_OK;
}
} // namespace

// Two device conditions are not caller errors and are answered by running the call again from scratch (results never
// depend on either): message buckets (and their overflow list) too small -- double the bucket capacity and re-plan the
// workspace; a team of k_push_team that waited too long for a member (its workgroups were not co-resident: another
// context's kernels held CUs) -- the next calls push with the bucketed kernels.
constexpr int TEAM_SUSPEND_CALLS = 8;
template <class F> int with_bucket_retry(fora_ctx *c, F call) {
    if (!c) return call();
    BucketRetry &br = c->retry;
    const uint32_t scale0 = br.scale, scale0t = br.scale_topk;
    bool team_retried = false;
    auto forget_attempt = [&](const fora_timing &t0) { // the failed attempt must leave no trace in the timings: drop its event pairs and counters
        drop_pairs(c);
        c->tm.total = t0;
    };
    auto give_up = [&](int rc) { // the enlarged plan did not help: do not keep it; no pair of the failed call stays behind
        if (br.scale != scale0 || br.scale_topk != scale0t) {
            br.scale = scale0; br.scale_topk = scale0t;
            (void)hipSetDevice(c->device);
            free_workspace(c);
        }
        return drop_pairs_unless_ok(c, rc);
    };
    for (;;) {
        const fora_timing t0 = c->tm.total;
        const int rc = call();
        if (rc == FORA_OK && c->team_run.suspend > 0 && !team_retried) c->team_run.suspend--; // (a retried call has just started the count)
        if (rc == FORA_OK) return rc;
        if (rc != FORA_E_OVERFLOW) return give_up(rc);
        if (c->team_run.timeout_seen && !team_retried) {
            c->team_run.timeout_seen = false;
            c->team_run.suspend = TEAM_SUSPEND_CALLS;
            c->team_run.fallbacks++;
            team_retried = true;
            forget_attempt(t0);
            continue;
        }
        // the multiplier of the regime the call planned with (BucketRetry::div is set by the call itself)
        uint32_t &cur = br.div > 1 ? br.scale_topk : br.scale;
        if (!br.overflow || cur >= (1u << 16)) return give_up(rc);
        cur *= 2;
        br.retries++;
        br.overflow = false;
        forget_attempt(t0);
        free_workspace(c);
    }
}

// the words of the context that mirror an option
static void apply_options(fora_ctx *c) { c->tm.profiling = c->opt_.profile != 0; c->grid_blocks = c->opt_.grid > 0 ? (int)c->opt_.grid : 2048; }

// =============================================================================== the host drivers of the calls on the held rows
namespace {
// is p device memory of the ctx's GPU?  (host memory the runtime has never seen: no attributes, or "unregistered")
int sparse_dest(fora_ctx *c, const void *p, bool &on_device) {
    hipPointerAttribute_t a{};
    on_device = false;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return FORA_OK; }
    if (a.type != hipMemoryTypeDevice) return FORA_OK;
    if (a.device != c->device) return fail(c, FORA_E_ARG, "destination is memory of another GPU");
    on_device = true;
    return FORA_OK;
}

// e held words (device) as doubles into vals, on the ctx's stream: converted in place for device memory, SP_STAGE at a time
// through the sparse result's stage buffer for a host array
int fetch_vals(fora_ctx *c, const uint64_t *words, uint64_t e, double *vals, bool vals_on_device) {
    constexpr uint64_t SP_STAGE = 1ull << 22; // doubles converted on the device per copy to a host array
    const auto grid = [&](uint64_t cnt) { return dim3((unsigned)std::min<uint64_t>((cnt + BLOCK - 1) / BLOCK, 4096)); };
    if (vals_on_device) {
        hipLaunchKernelGGL(k_sparse_vals, grid(e), dim3(BLOCK), 0, c->stream, words, e, vals);
        return FORA_OK;
    }
    HIPCHK(c, c->sp.d_stage.ensure(SP_STAGE));
    for (uint64_t at = 0; at < e; at += SP_STAGE) {
        const uint64_t len = std::min(SP_STAGE, e - at);
        hipLaunchKernelGGL(k_sparse_vals, grid(len), dim3(BLOCK), 0, c->stream, words + at, len, c->sp.d_stage.get());
        HIPCHK(c, hipMemcpyAsync(vals + at, c->sp.d_stage.get(), len * 8, hipMemcpyDeviceToHost, c->stream));
    }
    return FORA_OK;
}

// ---- the frame of a call on the held rows: its operands, its outputs, the choice of a kernel, its begin and end
// a grown-or-kept buffer of the call; no room is FORA_E_NOMEM and leaves no sticky HIP error behind
template <typename T> int prop_ensure(fora_ctx *c, DevBuf<T> &b, size_t cnt, const char *what) {
    if (b.ensure(std::max<size_t>(cnt, 1)) == hipSuccess) return FORA_OK;
    (void)hipGetLastError();
    return fail(c, FORA_E_NOMEM, std::string("no device memory for ") + what);
}
// An operand of the caller's: a strided matrix or a per-entry vector, in host memory or on the ctx's GPU.  resolve() before
// anything is built, stage() among the call's buffers; ptr() is then what the launches read.  A null operand stays null.
struct HeldIn {
    const void *p = nullptr; uint64_t bytes = 0; bool dev = false;
    static HeldIn matrix(const void *p, uint64_t rows, int64_t ld, uint64_t width, uint32_t elt) { return HeldIn{p, prop_matrix_bytes(rows, (uint64_t)ld, width, elt)}; }
    static HeldIn vector(const void *p, uint64_t count, uint32_t elt) { return HeldIn{p, prop_vector_bytes(count, elt)}; }
    int resolve(fora_ctx *c) { return p ? sparse_dest(c, p, dev) : FORA_OK; }
    // a host operand into buf (`what` names it when there is no room); nothing to do on the device, or without entries
    int stage(fora_ctx *c, DevBuf<unsigned char> &buf, const char *what) {
        if (!p || dev || !c->sp.entries) return FORA_OK;
        if (int rc = prop_ensure(c, buf, (size_t)bytes, what)) return rc;
        HIPCHK(c, hipMemcpy(buf.get(), p, (size_t)bytes, hipMemcpyHostToDevice));
        p = buf.get();
        return FORA_OK;
    }
    const void *ptr() const { return p; }
    int32_t on_device() const { return dev ? 1 : 0; } // (the caller's pointer: the stats)
};
// An output of the caller's: rows x width of T at pitch ld; a per-entry vector is vector(): one row without a pitch.  resolve(),
// then reserve() among the call's buffers; the launches write ptr() at pitch ld() -- the caller's own memory and pitch on the
// device, a dense staging buffer for a host array, which fetch() copies out after the last launch (with a pitch: row by row,
// what lies between the rows stays the caller's).  A null output stays null throughout.
template <typename T> struct HeldOut {
    T *out = nullptr; int64_t pitch = 0; uint64_t rows = 0, width = 0; bool dev = false; T *work = nullptr;
    static HeldOut vector(T *out, uint64_t count) { return HeldOut{out, 0, 1, count}; }
    int resolve(fora_ctx *c) { work = out; return out ? sparse_dest(c, out, dev) : FORA_OK; }
    int reserve(fora_ctx *c, DevBuf<T> &staging) {
        if (!out || dev) return FORA_OK;
        if (int rc = prop_ensure(c, staging, (size_t)(rows * width), "a staged output")) return rc;
        work = staging.get();
        return FORA_OK;
    }
    T *ptr() const { return work; }
    T *ptr(uint64_t col) const { return work ? work + col : nullptr; } // (a head's columns)
    int64_t ld() const { return dev ? pitch : (int64_t)width; }
    int fetch(fora_ctx *c) const {
        if (!out || dev || !rows || !width) return FORA_OK;
        if (!pitch) HIPCHK(c, hipMemcpyAsync(out, work, (size_t)width * sizeof(T), hipMemcpyDeviceToHost, c->stream));
        else HIPCHK(c, hipMemcpy2DAsync(out, (size_t)pitch * sizeof(T), work, (size_t)width * sizeof(T), (size_t)width * sizeof(T), (size_t)rows, hipMemcpyDeviceToHost, c->stream));
        return FORA_OK;
    }
};
// The element types of the dense operands are those of fora_narrow.h, which also says how many bytes each takes (elt_bytes)
static_assert(ELT_F32 == FORA_PROP_F32 && ELT_BF16 == FORA_PROP_BF16 && ELT_F16 == FORA_PROP_F16 && ELT_E4M3 == FORA_PROP_E4M3 && ELT_E5M2 == FORA_PROP_E5M2,
              "fora_narrow.h and include/fora_hip.h name one set of element types");
template <int N> using int_c = std::integral_constant<int, N>;
// f(int_c<ET>, int_c<V>): the instantiation for an element type and one of the three vector widths that prop_geom /
// attn_vec_width took from prop_widths_bytes(elt_bytes(et)) -- a load site of V elements a lane, whose layout hangs on the type
template <int ET, typename F> void with_vec_of(uint32_t V, F &&f) {
    constexpr int wide = 16 / (int)elt_bytes(ET), mid = elt_bytes(ET) == 4 ? 2 : 4;
    if (V == (uint32_t)wide) f(int_c<ET>{}, int_c<wide>{});
    else if (V == (uint32_t)mid) f(int_c<ET>{}, int_c<mid>{});
    else f(int_c<ET>{}, int_c<1>{});
}
template <typename F> void with_vec(int et, uint32_t V, F &&f) {
    switch (et) {
        case ELT_F32: with_vec_of<ELT_F32>(V, f); break;
        case ELT_BF16: with_vec_of<ELT_BF16>(V, f); break;
        case ELT_F16: with_vec_of<ELT_F16>(V, f); break;
        case ELT_E4M3: with_vec_of<ELT_E4M3>(V, f); break;
        default: with_vec_of<ELT_E5M2>(V, f); break;
    }
}
// f(int_c<A>, int_c<B>) for the two operands of a one-element-per-lane load site (sddmm_load): the four compiled-in pairs of
// f32 and bf16, and one class, ELT_ANY for both, that reads the types at run time when either is a narrow one
template <typename F> void with_elt_pair(int a, int b, F &&f) {
    const bool a_old = a == ELT_F32 || a == ELT_BF16, b_old = b == ELT_F32 || b == ELT_BF16;
    if (!a_old || !b_old) f(int_c<ELT_ANY>{}, int_c<ELT_ANY>{});
    else if (a == ELT_BF16) { if (b == ELT_BF16) f(int_c<ELT_BF16>{}, int_c<ELT_BF16>{}); else f(int_c<ELT_BF16>{}, int_c<ELT_F32>{}); }
    else { if (b == ELT_BF16) f(int_c<ELT_F32>{}, int_c<ELT_BF16>{}); else f(int_c<ELT_F32>{}, int_c<ELT_F32>{}); }
}
// f(int_c<A>, int_c<B>, int_c<ET>, int_c<V>) for a fused kernel with a pair of one-element-per-lane operands and a vector one:
// the 24 instantiations of old while all three types are f32 or bf16; with a narrow type anywhere, ELT_ANY for the pair and
// the vector operand's own type -- 15 more, not 5 * 5 * 15
template <typename F> void with_fused_types(int a, int b, int vt, uint32_t V, F &&f) {
    const auto old = [](int t) { return t == ELT_F32 || t == ELT_BF16; };
    if (!old(a) || !old(b) || !old(vt)) with_vec(vt, V, [&](auto E, auto W) { f(int_c<ELT_ANY>{}, int_c<ELT_ANY>{}, E, W); });
    else with_elt_pair(a, b, [&](auto A, auto B) {
        if (vt == ELT_BF16) with_vec_of<ELT_BF16>(V, [&](auto E, auto W) { f(A, B, E, W); });
        else with_vec_of<ELT_F32>(V, [&](auto E, auto W) { f(A, B, E, W); });
    });
}
// f(std::bool_constant<a>, std::bool_constant<b>)
template <typename F> void with_bools(bool a, bool b, F &&f) {
    if (a) { if (b) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
    else { if (b) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
}
// the checks every entry point shares, under the call's name `who`; each keeps the checks that are its own
int held_call_begin(fora_ctx *c, const char *who, const int64_t *row_ptr, int nq) {
    if (!c) return FORA_E_ARG;
    if (!c->sp.valid) return fail(c, FORA_E_ARG, "no sparse result is held");
    if (nq < 0 || !row_ptr) return fail(c, FORA_E_ARG, std::string(who) + ": negative nq or null row_ptr");
    if (!prop_row_ptr_ok(row_ptr, nq, c->sp.entries)) return fail(c, FORA_E_ARG, std::string(who) + ": row_ptr is not the held result's");
    return FORA_OK;
}
// the end of a call: the stream idle, a failed launch or copy reported under the call's name; collect: the event times read
int held_call_end(fora_ctx *c, const char *who, bool collect = true) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(c, FORA_E_HIP, std::string(who) + ": " + hipGetErrorString(err));
    if (collect) ev_collect(c);
    return FORA_OK;
}

// ---- PROPAGATE and PROPAGATE, TRANSPOSED
// One side of the product: which output rows are summed over which entries.  Forward: the held rows (ids: nodes, feat: the n
// feature rows).  Transposed: the columns of the transposition (ids: the rows the entries came from, feat: the nq gradient rows).
struct PropSide {
    const int64_t *row_ptr; int rows;        // (host) the output rows' entries
    const int32_t *ids; const uint64_t *fix; // (device) the entries
    const uint64_t *rsum;                    // transposed and normalised: S by id, every weight divided by it in the gather; else null
    bool divide;                             // forward and normalised: a row's sum divided by its word sum in the combine
    const void *values = nullptr; bool val64 = false; // PROPAGATE WITH VALUES: the weights (device; null: the words), f64 or f32
    const int64_t *pos = nullptr;            // (device) with values, transposed: the held place of every entry; forward: null
    bool unit = false;                       // SUBGRAPH PRODUCTS without values: every weight 1.0, fix is not read
};
struct PropRunStats { uint64_t segments = 0, max_row = 0; int32_t chunks = 0, feat_on_device = 0; };

template <int ET, int V>
void prop_launch_gather(fora_ctx *c, const PropGeom &g, const PropSeg *segs, uint64_t nseg, const PropSide &sd, const void *feat, int64_t ldf, int d, double *part, uint64_t *segsum) {
    const uint64_t per_wg = (uint64_t)g.segs_per_wave * (BLOCK / 64);
    const dim3 grid((unsigned)((nseg + per_wg - 1) / per_wg), g.tiles);
    if (sd.values) with_bools(sd.pos != nullptr, sd.val64, [&](auto POS, auto V64) {
        hipLaunchKernelGGL((k_prop_gather_vals<ET, V, POS.value, V64.value>), grid, dim3(BLOCK), 0, c->stream, segs, nseg, sd.ids, sd.values, sd.pos, feat, ldf, (uint32_t)d, g.G, part);
    });
    else if (sd.unit) hipLaunchKernelGGL((k_sub_gather_one<ET, V>), grid, dim3(BLOCK), 0, c->stream, segs, nseg, sd.ids, feat, ldf, (uint32_t)d, g.G, part);
    else if (sd.rsum) hipLaunchKernelGGL((k_prop_gather_t<ET, V>), grid, dim3(BLOCK), 0, c->stream, segs, nseg, sd.ids, sd.fix, feat, ldf, (uint32_t)d, g.G, part, sd.rsum);
    else hipLaunchKernelGGL((k_prop_gather<ET, V>), grid, dim3(BLOCK), 0, c->stream, segs, nseg, sd.ids, sd.fix, feat, ldf, (uint32_t)d, g.G, part, segsum);
}
// the two kernels chunk by chunk over a plan whose segments and records lie at d_segs and d_recs: the partial sums of one chunk
// live at a time in the ctx's buffers, which the caller has ensured.  timed: an event pair per launch (PROPAGATE's own stats);
// a caller with a span of its own around the whole passes false.
void prop_launch_chunks(fora_ctx *c, const PropPlan &plan, const PropSeg *d_segs, const PropRowRec *d_recs, const PropSide &sd, int et, const PropGeom &g,
                        const void *feat, int64_t ldf, int d, uint64_t *segsum, float *w32, int64_t ld32, double *w64, int64_t ld64, bool timed,
                        const int64_t *mean_ptr = nullptr) { // (mean_ptr, device: FORA_SUB_MEAN -- a finished row divided by its number of entries)
    PropBufs &b = c->pr;
    for (size_t ci = 0; ci < plan.chunks.size(); ci++) {
        const PropChunk &ch = plan.chunks[ci];
        if (ch.nseg) {
            EvSpan ev(c);
            if (timed) ev.begin(EV_PROP_GATHER);
            const PropSeg *segs = d_segs + ch.seg0;
            with_vec(et, g.V, [&](auto E, auto V) { prop_launch_gather<E.value, V.value>(c, g, segs, ch.nseg, sd, feat, ldf, d, b.d_part.get(), segsum); });
        }
        if (ch.nrec) {
            EvSpan ev(c);
            if (timed) ev.begin(EV_PROP_COMBINE);
            const uint32_t rpb = d < BLOCK ? (uint32_t)(BLOCK / d) : 1u; // whole records per workgroup when a record is narrower than one
            const dim3 grid((unsigned)((d + BLOCK - 1) / BLOCK), (unsigned)std::min<uint64_t>((ch.nrec + rpb - 1) / rpb, 65535));
            const auto combine = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), 0, c->stream, d_recs + ch.rec0, ch.nrec,
                                   (uint32_t)d, rpb, (const double *)b.d_part.get(), (const uint64_t *)segsum, (const double *)b.d_carry.part(ci & 1, (size_t)d), b.d_carry.part(~ci & 1, (size_t)d),
                                   (const uint64_t *)b.d_scarry.part(ci & 1, 1), b.d_scarry.part(~ci & 1, 1), w32, ld32, w64, ld64, mean_ptr);
            };
            if (mean_ptr) combine(k_prop_combine<true>); else combine(k_prop_combine<false>);
        }
    }
}
// the product of one side with feat: plan, buffers, the two kernels chunk by chunk, the staged outputs; the stream is idle and
// the event times are collected when it returns FORA_OK
// every operand and output of a call asked where it lives, before anything is built: memory of another GPU is refused first
template <typename... O> int held_resolve(fora_ctx *c, O &...o) {
    int rc = FORA_OK;
    (void)(((rc = o.resolve(c)) != FORA_OK) || ...);
    return rc;
}
template <typename... O> int held_fetch(fora_ctx *c, const O &...o) { // the staged outputs copied out, after the last launch
    int rc = FORA_OK;
    (void)(((rc = o.fetch(c)) != FORA_OK) || ...);
    return rc;
}
// the product of one side with feat (resolved, as values and the outputs are): plan, buffers, the two kernels chunk by chunk, the
// staged outputs; the stream is idle and the event times are collected when it returns FORA_OK
int prop_run(fora_ctx *c, const PropSide &side, HeldIn feat, HeldIn values, int et, int d, int64_t ldf, HeldOut<float> o32, HeldOut<double> o64, PropRunStats &rs) {
    PropSide sd = side;
    const int nq = sd.rows;
    PropBufs &b = c->pr;
    // ---- the plan: chunks of prop_segs segments; 0: a quarter of the free memory in partial sums at most
    const uint64_t total = prop_segments(sd.row_ptr, nq);
    size_t fr = 0, tot = 0;
    if (c->opt_.prop_segs <= 0) HIPCHK(c, hipMemGetInfo(&fr, &tot));
    const uint64_t per = prop_chunk_segs(c->opt_.prop_segs, total, (uint64_t)fr, d);
    const PropPlan plan = prop_plan(sd.row_ptr, nq, per);
    // ---- every buffer of the call before the first launch: a call that finds no room has written nothing
    if (int rc = feat.stage(c, b.d_feat, "the feature upload")) return rc;
    if (int rc = values.stage(c, b.d_vals, "the values upload")) return rc;
    sd.values = values.ptr();
    if (int rc = prop_ensure(c, b.d_segs, plan.segs.size(), "the segment table")) return rc;
    if (int rc = prop_ensure(c, b.d_recs, plan.recs.size(), "the segment table")) return rc;
    if (int rc = prop_ensure(c, b.d_part, (size_t)(per * (uint64_t)d), "the partial sums")) return rc;
    if (int rc = prop_ensure(c, b.d_segsum, (size_t)per, "the partial sums")) return rc;
    if (int rc = prop_ensure(c, b.d_carry, 2 * (size_t)d, "the partial sums")) return rc;
    if (int rc = prop_ensure(c, b.d_scarry, 2, "the partial sums")) return rc;
    if (int rc = o32.reserve(c, b.d_out32)) return rc;
    if (int rc = o64.reserve(c, b.d_out64)) return rc;
    if (!plan.segs.empty()) HIPCHK(c, hipMemcpy(b.d_segs.get(), plan.segs.data(), plan.segs.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(b.d_recs.get(), plan.recs.data(), plan.recs.size() * sizeof(PropRowRec), hipMemcpyHostToDevice));
    const PropGeom g = prop_geom((uint64_t)(uintptr_t)feat.ptr(), ldf, d, elt_bytes(et), prop_widths_bytes(elt_bytes(et)), PROP_NWIDTHS);
    uint64_t *const segsum = sd.divide ? b.d_segsum.get() : nullptr;
    c->tm.prop_gather_ms = c->tm.prop_combine_ms = 0;
    prop_launch_chunks(c, plan, b.d_segs.get(), b.d_recs.get(), sd, et, g, feat.ptr(), ldf, d, segsum, o32.ptr(), o32.ld(), o64.ptr(), o64.ld(), true);
    if (int rc = held_fetch(c, o32, o64)) return rc;
    if (int rc = held_call_end(c, "sparse propagate")) return rc;
    rs.segments = total; rs.max_row = plan.max_row; rs.chunks = (int32_t)plan.chunks.size(); rs.feat_on_device = feat.on_device();
    return FORA_OK;
}
// the operands and outputs of the two products: feat of feat_rows rows, values per entry, out of out_rows rows
struct PropIO { HeldIn feat, values; HeldOut<float> o32; HeldOut<double> o64; };
PropIO prop_io(fora_ctx *c, const void *feat, int et, uint64_t feat_rows, int64_t ldf, int d, const void *values, int val_type, float *out32, double *out64,
               uint64_t out_rows, int64_t ldo) {
    return PropIO{HeldIn::matrix(feat, feat_rows, ldf, (uint64_t)d, elt_bytes(et)), HeldIn::vector(values, c->sp.entries, val_type == FORA_PROP_F64 ? 8 : 4),
                  HeldOut<float>{out32, ldo, out_rows, (uint64_t)d}, HeldOut<double>{out64, ldo, out_rows, (uint64_t)d}};
}
int prop_impl(fora_ctx *c, const int64_t *row_ptr, int nq, const void *feat, int feat_type, int d, int64_t ldf, int flags, const void *values, int val_type,
              float *out32, double *out64, int64_t ldo, fora_prop_stats *ps) {
    PropIO io = prop_io(c, feat, feat_type, held_cols(c), ldf, d, values, val_type, out32, out64, (uint64_t)nq, ldo);
    if (int rc = held_resolve(c, io.values, io.feat, io.o32, io.o64)) return rc;
    const PropSide sd{row_ptr, nq, c->sp.d_ids.get(), c->sp.d_fix.get(), nullptr, (flags & FORA_PROP_NORMALIZE) != 0, values, val_type == FORA_PROP_F64, nullptr};
    PropRunStats rs;
    if (int rc = prop_run(c, sd, io.feat, io.values, feat_type, d, ldf, io.o32, io.o64, rs)) return rc;
    if (ps) {
        ps->entries = c->sp.entries; ps->segments = rs.segments; ps->max_row = rs.max_row;
        ps->feat_bytes = c->sp.entries * (uint64_t)d * elt_bytes(feat_type);
        ps->chunks = rs.chunks; ps->feat_on_device = rs.feat_on_device;
        ps->gather_ms = c->tm.prop_gather_ms; ps->combine_ms = c->tm.prop_combine_ms;
    }
    return FORA_OK;
}

// ---- PROPAGATE, TRANSPOSED: the transposition of the held result (fora_propt.h, fora_propt_plan.h), built once per held result
int propt_build(fora_ctx *c, const int64_t *row_ptr, int nq) {
    const uint64_t entries = c->sp.entries, n = held_cols(c); // (the columns: the nodes, or the compacted result's own)
    PropTBufs t; // moved into the ctx after the last step; freed on every other way out
    DevBuf<uint32_t> d_cnt; PinBuf<uint32_t> h_cnt; // counts per node, then the cursors of the place pass; their pinned landing area
    DevBuf<uint64_t> d_key; DevBuf<int64_t> d_row_ptr; DevBuf<PropTRun> d_runs;
    // ---- every buffer before the first launch
    const char *what = "the transposition";
    if (int rc = prop_ensure(c, t.d_rows, (size_t)entries, what)) return rc;
    if (int rc = prop_ensure(c, t.d_fix, (size_t)entries, what)) return rc;
    if (int rc = prop_ensure(c, t.d_col_ptr, (size_t)n + 1, what)) return rc;
    if (int rc = prop_ensure(c, t.d_rsum, (size_t)nq, what)) return rc;
    if (int rc = prop_ensure(c, d_cnt, (size_t)n, what)) return rc;
    if (int rc = prop_ensure(c, d_key, (size_t)entries, what)) return rc;
    if (int rc = prop_ensure(c, d_row_ptr, (size_t)nq + 1, what)) return rc;
    if (int rc = prop_ensure(c, d_runs, (size_t)propt_max_runs(n, entries), what)) return rc;
    if (h_cnt.alloc((size_t)std::max<uint64_t>(n, 1)) != hipSuccess) { (void)hipGetLastError(); return fail(c, FORA_E_NOMEM, "no pinned memory for the transposition's counts"); }
    t.h_col_ptr.assign((size_t)n + 1, 0);
    t.nq = nq;
    c->tm.propt_transpose_ms = 0;
    if (entries) {
        const uint32_t wgs = (uint32_t)std::min<int>(nq, 65535);
        HIPCHK(c, hipMemcpy(d_row_ptr.get(), row_ptr, ((size_t)nq + 1) * 8, hipMemcpyHostToDevice));
        EvSpan ev(c, EV_PROPT_TRANSPOSE);
        HIPCHK(c, d_cnt.zero(c->stream, (size_t)n));
        HIPCHK(c, t.d_rsum.zero(c->stream, (size_t)nq));
        hipLaunchKernelGGL(k_propt_count, dim3(wgs), dim3(BLOCK), 0, c->stream, (const int64_t *)d_row_ptr.get(), (uint32_t)nq, (const int32_t *)c->sp.d_ids.get(),
                           (const uint64_t *)c->sp.d_fix.get(), (uint32_t)n, d_cnt.get(), reinterpret_cast<unsigned long long *>(t.d_rsum.get()));
        HIPCHK(c, hipMemcpyAsync(h_cnt.get(), d_cnt.get(), (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); // (the counts are back)
        if (propt_scan(h_cnt.get(), (int64_t)n, t.h_col_ptr.data()) != entries) return fail(c, FORA_E_HIP, "sparse transpose: the counts do not add up to the held entries");
        const PropTTiers tiers = propt_tiers(t.h_col_ptr.data(), (int64_t)n, c->opt_.propt_lds_cap);
        if (tiers.runs.size() > d_runs.size()) return fail(c, FORA_E_HIP, "sparse transpose: more runs than the table holds");
        t.columns = tiers.columns; t.max_col = tiers.max_col;
        t.short_cols = tiers.n_short; t.lds_cols = tiers.n_lds; t.global_cols = tiers.n_global;
        HIPCHK(c, hipMemcpyAsync(t.d_col_ptr.get(), t.h_col_ptr.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        if (!tiers.runs.empty()) HIPCHK(c, hipMemcpyAsync(d_runs.get(), tiers.runs.data(), tiers.runs.size() * sizeof(PropTRun), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, d_cnt.zero(c->stream, (size_t)n));
        hipLaunchKernelGGL(k_propt_place, dim3(wgs), dim3(BLOCK), 0, c->stream, (const int64_t *)d_row_ptr.get(), (uint32_t)nq, (const int32_t *)c->sp.d_ids.get(), (uint32_t)n,
                           (const int64_t *)t.d_col_ptr.get(), d_cnt.get(), d_key.get(), entries);
        const PropTRun *r_short = d_runs.get(), *r_lds = r_short + tiers.n_short, *r_global = r_lds + tiers.n_lds;
        if (tiers.n_short) hipLaunchKernelGGL(k_propt_sort_short, dim3((tiers.n_short + BLOCK / 64 - 1) / (BLOCK / 64)), dim3(BLOCK), 0, c->stream, r_short, tiers.n_short, d_key.get());
        if (tiers.n_lds) hipLaunchKernelGGL(k_propt_sort_lds, dim3(tiers.n_lds), dim3(BLOCK), 0, c->stream, r_lds, d_key.get());
        if (tiers.n_global) {
            const uint32_t P = propt_pow2(tiers.max_global);
            const unsigned gx = (unsigned)std::min<uint32_t>(std::max<uint32_t>(1, P / 2 / BLOCK), 1024);
            for (uint32_t r0 = 0; r0 < tiers.n_global; r0 += 65535) { // (a grid's y extent)
                const dim3 grid(gx, std::min<uint32_t>(65535, tiers.n_global - r0));
                for (uint32_t k = 2; k <= P; k <<= 1) {
                    hipLaunchKernelGGL(k_propt_sort_step, grid, dim3(BLOCK), 0, c->stream, r_global + r0, d_key.get(), k, 0u);
                    for (uint32_t j = k >> 2; j; j >>= 1) hipLaunchKernelGGL(k_propt_sort_step, grid, dim3(BLOCK), 0, c->stream, r_global + r0, d_key.get(), k, j);
                }
            }
        }
        hipLaunchKernelGGL(k_propt_fill, dim3((unsigned)std::min<uint64_t>((entries + BLOCK - 1) / BLOCK, 8192)), dim3(BLOCK), 0, c->stream, (const uint64_t *)d_key.get(), entries,
                           (const int64_t *)d_row_ptr.get(), (uint32_t)nq, (const uint64_t *)c->sp.d_fix.get(), t.d_rows.get(), t.d_fix.get());
        ev.end();
    } else {
        HIPCHK(c, t.d_col_ptr.zero(c->stream, (size_t)n + 1));
        HIPCHK(c, t.d_rsum.zero(c->stream));
    }
    if (int rc = held_call_end(c, "sparse transpose")) return rc; // (idle: h_col_ptr and the tables go out of use)
    t.built = true;
    c->pt = std::move(t);
    return FORA_OK;
}
// the transposition of the held result, built now unless it is there; row_ptr has passed prop_row_ptr_ok
int propt_ensure(fora_ctx *c, const int64_t *row_ptr, int nq, bool &built_now) {
    built_now = false;
    if (c->pt.built && c->pt.nq == nq) return FORA_OK;
    c->pt = PropTBufs{};
    if (int rc = propt_build(c, row_ptr, nq)) return rc;
    built_now = true;
    return FORA_OK;
}
// PROPAGATE WITH VALUES: pos of the transposition that is there, made once (k_propt_pos) and kept with it
int propt_ensure_pos(fora_ctx *c, const int64_t *row_ptr, int nq) {
    PropTBufs &t = c->pt;
    if (t.has_pos) return FORA_OK;
    const uint64_t entries = c->sp.entries;
    DevBuf<int64_t> d_pos, d_row_ptr;
    if (int rc = prop_ensure(c, d_pos, (size_t)entries, "the transposition's places")) return rc;
    if (int rc = prop_ensure(c, d_row_ptr, (size_t)nq + 1, "the transposition's places")) return rc;
    if (entries) {
        HIPCHK(c, hipMemcpy(d_row_ptr.get(), row_ptr, ((size_t)nq + 1) * 8, hipMemcpyHostToDevice));
        EvSpan ev(c, EV_PROPT_TRANSPOSE);
        hipLaunchKernelGGL(k_propt_pos, dim3((unsigned)std::min<uint64_t>((entries + BLOCK - 1) / BLOCK, 8192)), dim3(BLOCK), 0, c->stream, (const int64_t *)t.d_col_ptr.get(),
                           (uint32_t)held_cols(c), (const int32_t *)t.d_rows.get(), (const int64_t *)d_row_ptr.get(), (uint32_t)nq, (const int32_t *)c->sp.d_ids.get(), entries, d_pos.get());
        ev.end();
        if (int rc = held_call_end(c, "sparse transpose", false)) return rc; // (idle: d_row_ptr goes out of use; the span is collected with the product's)
    }
    t.d_pos = std::move(d_pos);
    t.has_pos = true;
    return FORA_OK;
}
int propt_impl(fora_ctx *c, const int64_t *row_ptr, int nq, const void *grad, int grad_type, int d, int64_t ldg, int flags, const void *values, int val_type,
               float *out32, double *out64, int64_t ldo, fora_propt_stats *ps) {
    PropIO io = prop_io(c, grad, grad_type, (uint64_t)nq, ldg, d, values, val_type, out32, out64, held_cols(c), ldo);
    if (int rc = held_resolve(c, io.feat, io.values, io.o32, io.o64)) return rc; // (before the transposition is built)
    bool built_now = false;
    if (int rc = propt_ensure(c, row_ptr, nq, built_now)) return rc;
    double transpose_ms = built_now ? c->tm.propt_transpose_ms : 0.0;
    if (values) if (int rc = propt_ensure_pos(c, row_ptr, nq)) return rc;
    const PropTBufs &t = c->pt;
    const PropSide sd{t.h_col_ptr.data(), (int)held_cols(c), t.d_rows.get(), t.d_fix.get(), (flags & FORA_PROP_NORMALIZE) ? t.d_rsum.get() : nullptr, false,
                      values, val_type == FORA_PROP_F64, values ? t.d_pos.get() : nullptr};
    PropRunStats rs;
    if (int rc = prop_run(c, sd, io.feat, io.values, grad_type, d, ldg, io.o32, io.o64, rs)) return rc;
    if (built_now) transpose_ms = c->tm.propt_transpose_ms; // (with values: the places too)
    if (ps) {
        ps->entries = c->sp.entries; ps->columns = t.columns; ps->segments = rs.segments; ps->max_col = t.max_col;
        ps->feat_bytes = c->sp.entries * (uint64_t)d * elt_bytes(grad_type);
        ps->chunks = rs.chunks; ps->feat_on_device = rs.feat_on_device; ps->built = built_now ? 1 : 0;
        if (built_now) { ps->short_cols = (int32_t)t.short_cols; ps->lds_cols = (int32_t)t.lds_cols; ps->global_cols = (int32_t)t.global_cols; }
        ps->transpose_ms = transpose_ms; ps->gather_ms = c->tm.prop_gather_ms; ps->combine_ms = c->tm.prop_combine_ms;
    }
    return FORA_OK;
}

// ---- SCORES (SDDMM)
template <int A_ET, int B_ET>
void sddmm_launch(fora_ctx *c, const PropSeg *segs, uint64_t nseg, const void *a, int64_t lda, const void *b, int64_t ldb, int d, uint32_t lg, float *o32, double *o64,
                  uint32_t types) {
    const uint64_t units = nseg * SDDMM_UNITS, per_wg = BLOCK / 64;
    hipLaunchKernelGGL((k_prop_sddmm<A_ET, B_ET>), dim3((unsigned)((units + per_wg - 1) / per_wg)), dim3(BLOCK), 0, c->stream, segs, nseg,
                       (const int32_t *)c->sp.d_ids.get(), a, lda, b, ldb, (uint32_t)d, lg, o32, o64, types);
}
// sddmm_launch for the element types of a and b
void sddmm_launch_for(int a_type, int b_type, fora_ctx *c, const PropSeg *segs, uint64_t nseg, const void *a, int64_t lda, const void *b, int64_t ldb, int d, uint32_t lg,
                      float *o32, double *o64) {
    with_elt_pair(a_type, b_type, [&](auto A, auto B) { sddmm_launch<A.value, B.value>(c, segs, nseg, a, lda, b, ldb, d, lg, o32, o64, sddmm_types(a_type, b_type)); });
}
int sddmm_impl(fora_ctx *c, const int64_t *row_ptr, int nq, const void *a_, int a_type, int64_t lda, const void *b_, int b_type, int64_t ldb, int d,
               float *out32, double *out64, fora_sddmm_stats *st) {
    const uint64_t entries = c->sp.entries;
    const uint32_t a_elt = elt_bytes(a_type), b_elt = elt_bytes(b_type);
    HeldIn a = HeldIn::matrix(a_, (uint64_t)nq, lda, (uint64_t)d, a_elt), b = HeldIn::matrix(b_, held_cols(c), ldb, (uint64_t)d, b_elt);
    HeldOut<float> o32 = HeldOut<float>::vector(out32, entries);
    HeldOut<double> o64 = HeldOut<double>::vector(out64, entries);
    if (int rc = held_resolve(c, a, b, o32, o64)) return rc;
    PropBufs &pb = c->pr;
    const uint64_t total = prop_segments(row_ptr, nq);
    const PropPlan plan = prop_plan(row_ptr, nq, std::max<uint64_t>(total, 1)); // (one chunk: there are no partial sums to hold)
    // ---- every buffer of the call before the launch: a call that finds no room has written nothing
    if (int rc = a.stage(c, pb.d_a, "the upload of a")) return rc;
    if (int rc = b.stage(c, pb.d_feat, "the upload of b")) return rc;
    if (int rc = prop_ensure(c, pb.d_segs, plan.segs.size(), "the segment table")) return rc;
    if (int rc = o32.reserve(c, pb.d_out32)) return rc;
    if (int rc = o64.reserve(c, pb.d_out64)) return rc;
    c->tm.sddmm_ms = 0;
    if (!plan.segs.empty()) {
        HIPCHK(c, hipMemcpy(pb.d_segs.get(), plan.segs.data(), plan.segs.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
        EvSpan ev(c, EV_SDDMM);
        sddmm_launch_for(a_type, b_type, c, pb.d_segs.get(), plan.segs.size(), a.ptr(), lda, b.ptr(), ldb, d, prop_group_lg((uint32_t)d), o32.ptr(), o64.ptr());
    }
    if (int rc = held_fetch(c, o32, o64)) return rc;
    if (int rc = held_call_end(c, "sparse sddmm")) return rc;
    if (st) {
        st->entries = entries; st->segments = total; st->max_row = plan.max_row;
        st->bytes = entries * (uint64_t)d * (a_elt + b_elt);
        st->a_on_device = a.on_device(); st->b_on_device = b.on_device();
        st->sddmm_ms = c->tm.sddmm_ms;
    }
    return FORA_OK;
}


// ---- ROW SOFTMAX
struct SoftmaxWork { const PropSeg *shrt, *lng; uint64_t n_short, n_long; double *seg_max, *part; uint32_t *nan_rows; };
inline dim3 softmax_grid(uint64_t nseg) { return dim3((unsigned)((nseg + BLOCK / 64 - 1) / (BLOCK / 64))); }
template <typename TS>
void softmax_launch(fora_ctx *c, const SoftmaxWork &w, const void *scores, double scale, float *o32, double *o64) {
    const TS *x = (const TS *)scores;
    if (w.n_short) hipLaunchKernelGGL((k_softmax_short<TS>), softmax_grid(w.n_short), dim3(BLOCK), 0, c->stream, w.shrt, w.n_short, x, scale, o32, o64, w.nan_rows);
    if (w.n_long) {
        hipLaunchKernelGGL((k_softmax_seg_max<TS>), softmax_grid(w.n_long), dim3(BLOCK), 0, c->stream, w.lng, w.n_long, x, scale, w.seg_max);
        hipLaunchKernelGGL((k_softmax_seg_sum<TS>), softmax_grid(w.n_long), dim3(BLOCK), 0, c->stream, w.lng, w.n_long, x, scale, (const double *)w.seg_max, w.part);
        hipLaunchKernelGGL((k_softmax_div<TS>), softmax_grid(w.n_long), dim3(BLOCK), 0, c->stream, w.lng, w.n_long, x, scale, (const double *)w.seg_max,
                           (const double *)w.part, o32, o64, w.nan_rows);
    }
}
template <typename TY, typename TG>
void softmax_bwd_launch(fora_ctx *c, const SoftmaxWork &w, const void *y, const void *g, double scale, float *o32, double *o64) {
    const TY *yy = (const TY *)y;
    const TG *gg = (const TG *)g;
    if (w.n_short) hipLaunchKernelGGL((k_softmax_bwd_short<TY, TG>), softmax_grid(w.n_short), dim3(BLOCK), 0, c->stream, w.shrt, w.n_short, yy, gg, scale, o32, o64);
    if (w.n_long) {
        hipLaunchKernelGGL((k_softmax_bwd_seg_sum<TY, TG>), softmax_grid(w.n_long), dim3(BLOCK), 0, c->stream, w.lng, w.n_long, yy, gg, w.part);
        hipLaunchKernelGGL((k_softmax_bwd_div<TY, TG>), softmax_grid(w.n_long), dim3(BLOCK), 0, c->stream, w.lng, w.n_long, yy, gg, scale, (const double *)w.part, o32, o64);
    }
}
// both calls: in = scores (forward) or y (backward), grad = null (forward) or g
int softmax_impl(fora_ctx *c, const int64_t *row_ptr, int nq, const void *in_, int in_type, const void *grad_, int g_type, double scale,
                 float *out32, double *out64, fora_softmax_stats *st) {
    const uint64_t entries = c->sp.entries;
    const bool bwd = grad_ != nullptr, in64 = in_type == FORA_PROP_F64, g64 = g_type == FORA_PROP_F64;
    HeldIn in = HeldIn::vector(in_, entries, in64 ? 8 : 4), grad = HeldIn::vector(grad_, entries, g64 ? 8 : 4);
    HeldOut<float> o32 = HeldOut<float>::vector(out32, entries);
    HeldOut<double> o64 = HeldOut<double>::vector(out64, entries);
    if (int rc = held_resolve(c, in, grad, o32, o64)) return rc;
    PropBufs &pb = c->pr;
    const uint64_t total = prop_segments(row_ptr, nq);
    const PropPlan plan = prop_plan(row_ptr, nq, std::max<uint64_t>(total, 1)); // (one chunk: the partials are a few bytes per segment)
    const SoftmaxLists lists = softmax_lists(plan.segs, row_ptr, softmax_short_cap(c->opt_.softmax_short));
    // ---- every buffer of the call before the first launch: a call that finds no room has written nothing
    if (int rc = in.stage(c, pb.d_vals, bwd ? "the upload of y" : "the upload of the scores")) return rc;
    if (int rc = grad.stage(c, pb.d_a, "the upload of grad")) return rc;
    if (int rc = prop_ensure(c, pb.d_segs, lists.segs.size(), "the segment table")) return rc;
    if (int rc = prop_ensure(c, pb.d_smax, 2 * (size_t)lists.n_long, "the segment maxima and sums")) return rc;
    if (int rc = prop_ensure(c, pb.d_smax_nan, 1, "the segment maxima and sums")) return rc;
    if (int rc = o32.reserve(c, pb.d_out32)) return rc;
    if (int rc = o64.reserve(c, pb.d_out64)) return rc;
    c->tm.softmax_ms = 0;
    uint32_t nan_rows = 0;
    if (!lists.segs.empty()) {
        HIPCHK(c, hipMemcpy(pb.d_segs.get(), lists.segs.data(), lists.segs.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
        const SoftmaxWork w{pb.d_segs.get(), pb.d_segs.get() + lists.n_short, lists.n_short, lists.n_long, pb.d_smax.get(), pb.d_smax.get() + lists.n_long, pb.d_smax_nan.get()};
        if (!bwd) HIPCHK(c, pb.d_smax_nan.zero(c->stream, 1));
        {
            EvSpan ev(c, EV_SOFTMAX);
            if (bwd) with_bools(in64, g64, [&](auto Y64, auto G64) {
                softmax_bwd_launch<std::conditional_t<Y64.value, double, float>, std::conditional_t<G64.value, double, float>>(c, w, in.ptr(), grad.ptr(), scale, o32.ptr(), o64.ptr());
            });
            else if (in64) softmax_launch<double>(c, w, in.ptr(), scale, o32.ptr(), o64.ptr());
            else softmax_launch<float>(c, w, in.ptr(), scale, o32.ptr(), o64.ptr());
        }
        if (!bwd) HIPCHK(c, hipMemcpyAsync(&nan_rows, pb.d_smax_nan.get(), sizeof(nan_rows), hipMemcpyDeviceToHost, c->stream));
    }
    if (int rc = held_fetch(c, o32, o64)) return rc;
    if (int rc = held_call_end(c, "sparse softmax")) return rc;
    if (st) {
        st->entries = entries; st->segments = total; st->max_row = plan.max_row;
        st->nan_rows = nan_rows; st->short_rows = lists.short_rows; st->long_rows = lists.long_rows;
        st->in_on_device = in.on_device(); st->grad_on_device = grad.on_device();
        st->softmax_ms = c->tm.softmax_ms;
    }
    return FORA_OK;
}
// the frame of the two calls (who: the call's name in messages; grad / g_type: the backward call's)
int softmax_entry(fora_ctx *c, const char *who, const int64_t *row_ptr, int nq, const void *in, int in_type, bool bwd, const void *grad, int g_type, double scale,
                  float *out32, double *out64, uint64_t cap, fora_softmax_stats *st) {
    if (int rc = held_call_begin(c, who, row_ptr, nq)) return rc;
    const std::string w = std::string(who) + ": ";
    if (in_type != FORA_PROP_F32 && in_type != FORA_PROP_F64) return fail(c, FORA_E_ARG, w + "an element type that is neither f32 nor f64");
    if (bwd && g_type != FORA_PROP_F32 && g_type != FORA_PROP_F64) return fail(c, FORA_E_ARG, w + "an element type that is neither f32 nor f64");
    if (!std::isfinite(scale)) return fail(c, FORA_E_ARG, w + "scale is not finite");
    if (!out32 && !out64) return fail(c, FORA_E_ARG, w + "no output");
    if (cap < c->sp.entries) return fail(c, FORA_E_ARG, w + "cap is smaller than the held result");
    if (c->sp.entries && (!in || (bwd && !grad))) return fail(c, FORA_E_ARG, w + "null input");
    if (st) memset(st, 0, sizeof(*st));
    if (nq == 0) return FORA_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return drop_pairs_unless_ok(c, softmax_impl(c, row_ptr, nq, c->sp.entries ? in : nullptr, in_type, bwd && c->sp.entries ? grad : nullptr, g_type, scale, out32, out64, st));
}

// ---- ATTENTION
template <int QE, int KE, int VE, int V>
void attn_launch(fora_ctx *c, const PropSeg *rows, uint64_t nrow, int heads, const void *q, int64_t ldq, const void *k, int64_t ldk, const void *v, int64_t ldv,
                 int d, int dv, uint32_t lg, double scale, uint64_t entries, float *o32, int64_t ld32, double *o64, int64_t ld64, float *y32, double *y64, uint32_t *nan_rows, uint32_t types) {
    const uint64_t units = nrow * (uint64_t)heads;
    hipLaunchKernelGGL((k_attn_short<QE, KE, VE, V>), dim3((unsigned)((units + ATTN_ROWS - 1) / ATTN_ROWS)), dim3(BLOCK), 0, c->stream, rows, nrow, (uint32_t)heads,
                       (const int32_t *)c->sp.d_ids.get(), q, ldq, k, ldk, v, ldv, (uint32_t)d, (uint32_t)dv, lg, scale, entries, o32, ld32, o64, ld64, y32, y64, nan_rows, types);
}
inline const void *attn_cols(const void *m, uint64_t col, uint32_t elt) { return (const unsigned char *)m + col * elt; }

int attention_impl(fora_ctx *c, const int64_t *row_ptr, int nq, const void *q_, int q_type, int64_t ldq, const void *k_, int k_type, int64_t ldk,
                   const void *v_, int v_type, int64_t ldv, int d, int dv, int heads, double scale, float *out32, double *out64, int64_t ldo,
                   float *y32_, double *y64_, fora_attn_stats *st) {
    const uint64_t entries = c->sp.entries, n = held_cols(c);
    const uint32_t q_elt = elt_bytes(q_type), k_elt = elt_bytes(k_type), v_elt = elt_bytes(v_type);
    const uint64_t wq = (uint64_t)heads * (uint64_t)d, wv = (uint64_t)heads * (uint64_t)dv; // columns of q and k; of v and out
    HeldIn q = HeldIn::matrix(q_, (uint64_t)nq, ldq, wq, q_elt), k = HeldIn::matrix(k_, n, ldk, wq, k_elt), v = HeldIn::matrix(v_, n, ldv, wv, v_elt);
    HeldOut<float> o32{out32, ldo, (uint64_t)nq, wv}, y32 = HeldOut<float>::vector(y32_, (uint64_t)heads * entries);
    HeldOut<double> o64{out64, ldo, (uint64_t)nq, wv}, y64 = HeldOut<double>::vector(y64_, (uint64_t)heads * entries);
    if (int rc = held_resolve(c, q, k, v, o32, o64, y32, y64)) return rc;
    PropBufs &pb = c->pr;
    // ---- the plan: the short rows' list; the longer rows' segments in chunks of prop_segs (0: a quarter of the free memory in
    // partial sums at most), split once more for the softmax kernels by softmax_short
    const uint32_t cap = attn_short_cap(c->opt_.attn_short);
    const uint64_t long_segs = prop_long_segments(row_ptr, nq, cap);
    size_t fr = 0, tot = 0;
    if (long_segs && c->opt_.prop_segs <= 0) HIPCHK(c, hipMemGetInfo(&fr, &tot));
    const uint64_t per = prop_chunk_segs(c->opt_.prop_segs, long_segs, (uint64_t)fr, dv);
    const AttnPlan plan = attn_plan(row_ptr, nq, cap, per);
    const SoftmaxLists sm = softmax_lists(plan.lng.segs, row_ptr, softmax_short_cap(c->opt_.softmax_short));
    const bool lng = !plan.lrows.empty();
    // ---- every buffer of the call before the first launch: a call that finds no room has written nothing
    if (int rc = q.stage(c, pb.d_a, "the upload of q")) return rc;
    if (int rc = k.stage(c, pb.d_feat, "the upload of k")) return rc;
    if (int rc = v.stage(c, pb.d_v, "the upload of v")) return rc;
    const size_t at_short = 0, at_lsegs = plan.shrt.size(), at_sm = at_lsegs + plan.lng.segs.size(), at_lrows = at_sm + sm.segs.size(),
                 nsegs = at_lrows + plan.lrows.size();
    if (int rc = prop_ensure(c, pb.d_segs, nsegs, "the segment table")) return rc;
    if (int rc = prop_ensure(c, pb.d_smax_nan, 1, "the segment maxima and sums")) return rc;
    if (lng) {
        if (int rc = prop_ensure(c, pb.d_recs, plan.lng.recs.size(), "the segment table")) return rc;
        if (int rc = prop_ensure(c, pb.d_part, (size_t)(per * (uint64_t)dv), "the partial sums")) return rc;
        if (int rc = prop_ensure(c, pb.d_carry, 2 * (size_t)dv, "the partial sums")) return rc;
        if (int rc = prop_ensure(c, pb.d_scarry, 2, "the partial sums")) return rc;
        if (int rc = prop_ensure(c, pb.d_smax, 2 * (size_t)sm.n_long, "the segment maxima and sums")) return rc;
        if (int rc = prop_ensure(c, pb.d_attn_s, (size_t)entries, "the scores of the longer rows")) return rc;
        if (!y64_) if (int rc = prop_ensure(c, pb.d_attn_y, (size_t)entries, "the y of the longer rows")) return rc;
    }
    if (int rc = o32.reserve(c, pb.d_out32)) return rc;
    if (int rc = o64.reserve(c, pb.d_out64)) return rc;
    if (int rc = y32.reserve(c, pb.d_y32)) return rc;
    if (int rc = y64.reserve(c, pb.d_y64)) return rc;
    PropSeg *const ds = pb.d_segs.get();
    if (!plan.shrt.empty()) HIPCHK(c, hipMemcpy(ds + at_short, plan.shrt.data(), plan.shrt.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
    if (lng) {
        HIPCHK(c, hipMemcpy(ds + at_lsegs, plan.lng.segs.data(), plan.lng.segs.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(ds + at_sm, sm.segs.data(), sm.segs.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(ds + at_lrows, plan.lrows.data(), plan.lrows.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(pb.d_recs.get(), plan.lng.recs.data(), plan.lng.recs.size() * sizeof(PropRowRec), hipMemcpyHostToDevice));
    }
    const uint32_t lg = prop_group_lg((uint32_t)d);
    const uint32_t *const widths = prop_widths_bytes(v_elt);
    c->tm.attn_ms = 0;
    uint32_t nan_rows = 0;
    HIPCHK(c, pb.d_smax_nan.zero(c->stream, 1));
    {
        EvSpan ev(c, EV_ATTN);
        if (!plan.shrt.empty())
            with_fused_types(q_type, k_type, v_type, attn_vec_width((uint64_t)(uintptr_t)v.ptr(), ldv, dv, heads, v_elt, widths, PROP_NWIDTHS), [&](auto QE, auto KE, auto VE, auto V) {
                attn_launch<QE.value, KE.value, VE.value, V.value>(c, ds + at_short, plan.shrt.size(), heads, q.ptr(), ldq, k.ptr(), ldk, v.ptr(), ldv, d, dv, lg, scale, entries,
                                                                   o32.ptr(), o32.ld(), o64.ptr(), o64.ld(), y32.ptr(), y64.ptr(), pb.d_smax_nan.get(), sddmm_types(q_type, k_type));
            });
        for (int h = 0; lng && h < heads; h++) { // the longer rows, one head at a time through the two per-entry buffers
            const void *qh = attn_cols(q.ptr(), (uint64_t)h * d, q_elt), *kh = attn_cols(k.ptr(), (uint64_t)h * d, k_elt), *vh = attn_cols(v.ptr(), (uint64_t)h * dv, v_elt);
            double *const s64 = pb.d_attn_s.get();
            double *const yh64 = y64.ptr() ? y64.ptr((uint64_t)h * entries) : pb.d_attn_y.get();
            float *const yh32 = y32.ptr((uint64_t)h * entries);
            const PropSeg *segs = ds + at_lsegs;
            sddmm_launch_for(q_type, k_type, c, segs, plan.lng.segs.size(), qh, ldq, kh, ldk, d, lg, nullptr, s64);
            const SoftmaxWork w{ds + at_sm, ds + at_sm + sm.n_short, sm.n_short, sm.n_long, pb.d_smax.get(), pb.d_smax.get() + sm.n_long, pb.d_smax_nan.get()};
            softmax_launch<double>(c, w, s64, scale, yh32, yh64);
            const PropSide sd{row_ptr, nq, c->sp.d_ids.get(), nullptr, nullptr, false, yh64, true, nullptr};
            const PropGeom g = prop_geom((uint64_t)(uintptr_t)vh, ldv, dv, v_elt, widths, PROP_NWIDTHS);
            float *const oh32 = o32.ptr((uint64_t)h * dv);
            double *const oh64 = o64.ptr((uint64_t)h * dv);
            prop_launch_chunks(c, plan.lng, segs, pb.d_recs.get(), sd, v_type, g, vh, ldv, dv, nullptr, oh32, o32.ld(), oh64, o64.ld(), false);
            const dim3 grid((unsigned)((dv + BLOCK - 1) / BLOCK), (unsigned)std::min<uint64_t>(plan.lrows.size(), 65535));
            hipLaunchKernelGGL(k_attn_nan_rows, grid, dim3(BLOCK), 0, c->stream, (const PropSeg *)(ds + at_lrows), (uint64_t)plan.lrows.size(), (const double *)yh64,
                               (uint32_t)dv, oh32, o32.ld(), oh64, o64.ld());
        }
    }
    HIPCHK(c, hipMemcpyAsync(&nan_rows, pb.d_smax_nan.get(), sizeof(nan_rows), hipMemcpyDeviceToHost, c->stream));
    if (int rc = held_fetch(c, o32, o64, y32, y64)) return rc;
    if (int rc = held_call_end(c, "sparse attention")) return rc;
    if (st) {
        st->entries = entries; st->segments = plan.segments; st->max_row = plan.max_row;
        st->nan_rows = nan_rows; st->short_rows = plan.short_rows; st->long_rows = plan.long_rows;
        st->q_on_device = q.on_device(); st->k_on_device = k.on_device(); st->v_on_device = v.on_device();
        st->attn_ms = c->tm.attn_ms;
    }
    return FORA_OK;
}

// ---- ATTENTION, BACKWARD
template <int GE, int VE, int KE, int V>
void attn_bwd_launch(fora_ctx *c, const PropSeg *rows, uint64_t nrow, int heads, const void *g, int64_t ldg, const void *v, int64_t ldv, const void *k, int64_t ldk,
                     int d, int dv, uint32_t lgv, double scale, uint64_t entries, const void *y, bool y_f64, double *ds, float *o32, int64_t ld32, double *o64, int64_t ld64,
                     uint32_t types) {
    const uint64_t units = nrow * (uint64_t)heads;
    hipLaunchKernelGGL((k_attn_bwd_short<GE, VE, KE, V>), dim3((unsigned)((units + ATTN_ROWS - 1) / ATTN_ROWS)), dim3(BLOCK), 0, c->stream, rows, nrow, (uint32_t)heads,
                       (const int32_t *)c->sp.d_ids.get(), g, ldg, v, ldv, k, ldk, (uint32_t)d, (uint32_t)dv, lgv, scale, entries, y, y_f64, ds, o32, ld32, o64, ld64, types);
}
template <int ET, int V>
void attn_cols_launch(fora_ctx *c, const PropGeom &g, const PropSeg *cols, uint64_t ncol, int heads, const void *values, bool val64, uint64_t entries,
                      const void *feat, int64_t ldf, int w, float *o32, int64_t ld32, double *o64, int64_t ld64) {
    const uint64_t units = ncol * (uint64_t)heads, per_wg = (uint64_t)g.segs_per_wave * (BLOCK / 64);
    const dim3 grid((unsigned)((units + per_wg - 1) / per_wg), g.tiles);
    const int32_t *rows = c->pt.d_rows.get();
    const int64_t *pos = c->pt.d_pos.get();
    if (val64) hipLaunchKernelGGL((k_attn_cols<ET, V, true>), grid, dim3(BLOCK), 0, c->stream, cols, ncol, (uint32_t)heads, rows, pos, values, entries, feat, ldf, (uint32_t)w, g.G, o32, ld32, o64, ld64);
    else hipLaunchKernelGGL((k_attn_cols<ET, V, false>), grid, dim3(BLOCK), 0, c->stream, cols, ncol, (uint32_t)heads, rows, pos, values, entries, feat, ldf, (uint32_t)w, g.G, o32, ld32, o64, ld64);
}
// +0.0 to an n x width output: one clear where the rows lie back to back, a clear per row band otherwise (a pitch wider than
// the output: what lies between the rows is the caller's)
template <typename T> hipError_t attn_zero(fora_ctx *c, T *out, int64_t ld, uint64_t rows, uint64_t width) {
    if (!out || !rows) return hipSuccess;
    if ((uint64_t)ld == width) return hipMemsetAsync(out, 0, rows * width * sizeof(T), c->stream);
    return hipMemset2DAsync(out, (size_t)ld * sizeof(T), 0, width * sizeof(T), rows, c->stream);
}
// one gradient of the column side: out[v][h * w + c] = the sum over column v's entries p of values[h * entries + pos[p]] *
// feat[rows[p]][h * w + c].  The outputs zeroed (the empty columns), the short columns of all heads in one launch, the longer
// ones head by head through PROPAGATE's kernels over the cached plan.
int attn_bwd_cols(fora_ctx *c, int heads, uint64_t entries, const void *values, bool val64, const void *feat, int et, int64_t ldf, int w,
                  float *o32, int64_t ld32, double *o64, int64_t ld64) {
    const PropTBufs &t = c->pt;
    const AttnColPlan &cp = t.cols.plan;
    const uint64_t n = held_cols(c);
    const uint32_t elt = elt_bytes(et);
    const uint32_t *const widths = prop_widths_bytes(elt);
    HIPCHK(c, attn_zero(c, o32, ld32, n, (uint64_t)heads * (uint64_t)w));
    HIPCHK(c, attn_zero(c, o64, ld64, n, (uint64_t)heads * (uint64_t)w));
    if (!cp.shrt.empty()) {
        const PropGeom g = attn_cols_geom(attn_vec_width((uint64_t)(uintptr_t)feat, ldf, w, heads, elt, widths, PROP_NWIDTHS), w);
        with_vec(et, g.V, [&](auto E, auto V) {
            attn_cols_launch<E.value, V.value>(c, g, t.cols.d_short.get(), cp.shrt.size(), heads, values, val64, entries, feat, ldf, w, o32, ld32, o64, ld64);
        });
    }
    for (int h = 0; cp.long_cols && h < heads; h++) {
        const void *fh = attn_cols(feat, (uint64_t)h * w, elt);
        const void *vh = (const unsigned char *)values + (uint64_t)h * entries * (val64 ? 8 : 4);
        const PropSide sd{t.h_col_ptr.data(), (int)n, t.d_rows.get(), nullptr, nullptr, false, vh, val64, t.d_pos.get()};
        const PropGeom g = prop_geom((uint64_t)(uintptr_t)fh, ldf, w, elt, widths, PROP_NWIDTHS);
        prop_launch_chunks(c, cp.lng, t.cols.d_lsegs.get(), t.cols.d_lrecs.get(), sd, et, g, fh, ldf, w, nullptr, o32 ? o32 + (uint64_t)h * w : nullptr, ld32,
                           o64 ? o64 + (uint64_t)h * w : nullptr, ld64, false);
    }
    return FORA_OK;
}

int attention_bwd_impl(fora_ctx *c, const int64_t *row_ptr, int nq, const void *q_, int q_type, int64_t ldq, const void *k_, int k_type, int64_t ldk,
                       const void *v_, int v_type, int64_t ldv, const void *g_, int g_type, int64_t ldg, const void *y_, int y_type,
                       int d, int dv, int heads, double scale, const fora_attn_grads &gr, fora_attn_bwd_stats *st) {
    const uint64_t entries = c->sp.entries, n = held_cols(c);
    const bool y_f64 = y_type == FORA_PROP_F64;
    const uint32_t q_elt = elt_bytes(q_type), k_elt = elt_bytes(k_type), v_elt = elt_bytes(v_type), g_elt = elt_bytes(g_type), y_elt = y_f64 ? 8 : 4;
    const uint64_t wq = (uint64_t)heads * (uint64_t)d, wv = (uint64_t)heads * (uint64_t)dv; // columns of q, k, dq and dk; of v, g and dv
    const bool want_dq = gr.dq32 || gr.dq64, want_dk = gr.dk32 || gr.dk64, want_dv = gr.dv32 || gr.dv64;
    const bool want_rows = want_dq || want_dk, want_cols = want_dk || want_dv; // dy and ds; the transposition
    HeldIn q = HeldIn::matrix(q_, (uint64_t)nq, ldq, wq, q_elt), k = HeldIn::matrix(k_, n, ldk, wq, k_elt), v = HeldIn::matrix(v_, n, ldv, wv, v_elt);
    HeldIn g = HeldIn::matrix(g_, (uint64_t)nq, ldg, wv, g_elt), y = HeldIn::vector(y_, (uint64_t)heads * entries, y_elt);
    HeldOut<float> dq32{gr.dq32, gr.lddq, (uint64_t)nq, wq}, dk32{gr.dk32, gr.lddk, n, wq}, dv32{gr.dv32, gr.lddv, n, wv};
    HeldOut<double> dq64{gr.dq64, gr.lddq, (uint64_t)nq, wq}, dk64{gr.dk64, gr.lddk, n, wq}, dv64{gr.dv64, gr.lddv, n, wv};
    if (int rc = held_resolve(c, q, k, v, g, y, dq32, dq64, dk32, dk64, dv32, dv64)) return rc; // (before the transposition is built)
    // ---- the transposition and its places, as the first transposed product with values would build them
    bool built_now = false;
    if (want_cols) {
        if (int rc = propt_ensure(c, row_ptr, nq, built_now)) return rc;
        if (int rc = propt_ensure_pos(c, row_ptr, nq)) return rc;
    }
    PropBufs &pb = c->pr;
    PropTBufs &t = c->pt;
    // ---- the plans.  Rows: as the forward call's, the longer rows' product d columns wide.  Columns: from the cache when "attn_short"
    // and the resolved chunk size are the ones it was made under
    const uint32_t cap = attn_short_cap(c->opt_.attn_short);
    const uint64_t long_row_segs = want_rows ? prop_long_segments(row_ptr, nq, cap) : 0;
    uint64_t long_col_segs = 0;
    if (want_cols) long_col_segs = t.cols.valid && t.cols.short_cap == cap ? t.cols.long_segs : attn_long_col_segs(t.h_col_ptr.data(), (int64_t)n, cap);
    size_t fr = 0, tot = 0;
    if ((long_row_segs || long_col_segs) && c->opt_.prop_segs <= 0) HIPCHK(c, hipMemGetInfo(&fr, &tot));
    const int wmax = std::max(d, dv);
    const uint64_t per_rows = prop_chunk_segs(c->opt_.prop_segs, long_row_segs, (uint64_t)fr, d);
    const uint64_t per_cols = prop_chunk_segs(c->opt_.prop_segs, long_col_segs, (uint64_t)fr, wmax);
    const AttnPlan plan = attn_plan(row_ptr, nq, cap, per_rows);
    const SoftmaxLists sm = softmax_lists(plan.lng.segs, row_ptr, softmax_short_cap(c->opt_.softmax_short));
    const bool lng_rows = want_rows && !plan.lrows.empty();
    const bool plan_cached = want_cols && t.cols.valid && t.cols.short_cap == cap && t.cols.chunk_segs == per_cols;
    if (want_cols && !plan_cached) {
        PropTBufs::ColPlan nc; // moved into the transposition when complete
        nc.short_cap = cap; nc.chunk_segs = per_cols; nc.long_segs = long_col_segs;
        nc.plan = attn_col_plan(t.h_col_ptr.data(), (int64_t)n, cap, per_cols);
        if (int rc = prop_ensure(c, nc.d_short, nc.plan.shrt.size(), "the column table")) return rc;
        if (int rc = prop_ensure(c, nc.d_lsegs, nc.plan.lng.segs.size(), "the column table")) return rc;
        if (int rc = prop_ensure(c, nc.d_lrecs, nc.plan.lng.recs.size(), "the column table")) return rc;
        if (!nc.plan.shrt.empty()) HIPCHK(c, hipMemcpy(nc.d_short.get(), nc.plan.shrt.data(), nc.plan.shrt.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
        if (!nc.plan.lng.segs.empty()) HIPCHK(c, hipMemcpy(nc.d_lsegs.get(), nc.plan.lng.segs.data(), nc.plan.lng.segs.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
        if (!nc.plan.lng.recs.empty()) HIPCHK(c, hipMemcpy(nc.d_lrecs.get(), nc.plan.lng.recs.data(), nc.plan.lng.recs.size() * sizeof(PropRowRec), hipMemcpyHostToDevice));
        nc.valid = true;
        t.cols = std::move(nc);
    }
    const bool lng_cols = want_cols && t.cols.plan.long_cols != 0;
    // ---- every buffer of the call before the first launch: a call that finds no room has written nothing.  An operand that no
    // wanted gradient reads is not uploaded
    if (want_dk) if (int rc = q.stage(c, pb.d_a, "the upload of q")) return rc;
    if (want_dq) if (int rc = k.stage(c, pb.d_feat, "the upload of k")) return rc;
    if (want_rows) if (int rc = v.stage(c, pb.d_v, "the upload of v")) return rc;
    if (int rc = g.stage(c, pb.d_g, "the upload of g")) return rc;
    if (int rc = y.stage(c, pb.d_vals, "the upload of y")) return rc;
    const size_t at_short = 0, at_lsegs = plan.shrt.size(), at_sm = at_lsegs + plan.lng.segs.size(), nsegs = at_sm + sm.segs.size();
    if (want_rows) if (int rc = prop_ensure(c, pb.d_segs, nsegs, "the segment table")) return rc;
    if (lng_rows) {
        if (int rc = prop_ensure(c, pb.d_recs, plan.lng.recs.size(), "the segment table")) return rc;
        if (int rc = prop_ensure(c, pb.d_smax, 2 * (size_t)sm.n_long, "the segment sums")) return rc;
        if (int rc = prop_ensure(c, pb.d_attn_s, (size_t)entries, "the dy of the longer rows")) return rc;
    }
    if (lng_rows || lng_cols) {
        const uint64_t part = std::max(lng_rows && want_dq ? per_rows * (uint64_t)d : 0, lng_cols ? per_cols * (uint64_t)wmax : 0);
        if (int rc = prop_ensure(c, pb.d_part, (size_t)part, "the partial sums")) return rc;
        if (int rc = prop_ensure(c, pb.d_carry, 2 * (size_t)wmax, "the partial sums")) return rc;
        if (int rc = prop_ensure(c, pb.d_scarry, 2, "the partial sums")) return rc;
    }
    if (want_dk || lng_rows) if (int rc = prop_ensure(c, pb.d_attn_ds, (size_t)heads * (size_t)entries, "ds")) return rc;
    if (int rc = dq32.reserve(c, pb.d_out32)) return rc;
    if (int rc = dq64.reserve(c, pb.d_out64)) return rc;
    if (int rc = dk32.reserve(c, pb.d_dk32)) return rc;
    if (int rc = dk64.reserve(c, pb.d_dk64)) return rc;
    if (int rc = dv32.reserve(c, pb.d_dv32)) return rc;
    if (int rc = dv64.reserve(c, pb.d_dv64)) return rc;
    PropSeg *const dsg = pb.d_segs.get();
    if (want_rows && !plan.shrt.empty()) HIPCHK(c, hipMemcpy(dsg + at_short, plan.shrt.data(), plan.shrt.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
    if (lng_rows) {
        HIPCHK(c, hipMemcpy(dsg + at_lsegs, plan.lng.segs.data(), plan.lng.segs.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(dsg + at_sm, sm.segs.data(), sm.segs.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(pb.d_recs.get(), plan.lng.recs.data(), plan.lng.recs.size() * sizeof(PropRowRec), hipMemcpyHostToDevice));
    }
    double *const ds = want_dk || lng_rows ? pb.d_attn_ds.get() : nullptr;
    const uint32_t lgv = prop_group_lg((uint32_t)dv); // (the dv columns of dy)
    const uint32_t *const widths_k = prop_widths_bytes(k_elt);
    c->tm.attn_ms = 0;
    {
        EvSpan ev(c, EV_ATTN);
        if (want_rows && !plan.shrt.empty()) // dy, ds and dq of the short rows, all heads
            with_fused_types(g_type, v_type, k_type, attn_vec_width((uint64_t)(uintptr_t)k.ptr(), ldk, d, heads, k_elt, widths_k, PROP_NWIDTHS), [&](auto GE, auto VE, auto KE, auto V) {
                attn_bwd_launch<GE.value, VE.value, KE.value, V.value>(c, dsg + at_short, plan.shrt.size(), heads, g.ptr(), ldg, v.ptr(), ldv, k.ptr(), ldk, d, dv, lgv, scale, entries,
                                                                       y.ptr(), y_f64, want_dk ? ds : nullptr, dq32.ptr(), dq32.ld(), dq64.ptr(), dq64.ld(), sddmm_types(g_type, v_type));
            });
        for (int h = 0; lng_rows && h < heads; h++) { // the longer rows, one head at a time: dy, ds into the head's slice, dq
            const void *gh = attn_cols(g.ptr(), (uint64_t)h * dv, g_elt), *vh = attn_cols(v.ptr(), (uint64_t)h * dv, v_elt), *kh = attn_cols(k.ptr(), (uint64_t)h * d, k_elt);
            const void *yh = (const unsigned char *)y.ptr() + (uint64_t)h * entries * y_elt;
            double *const dy64 = pb.d_attn_s.get(), *const dsh = ds + (uint64_t)h * entries;
            const PropSeg *segs = dsg + at_lsegs;
            sddmm_launch_for(g_type, v_type, c, segs, plan.lng.segs.size(), gh, ldg, vh, ldv, dv, lgv, nullptr, dy64);
            const SoftmaxWork w{dsg + at_sm, dsg + at_sm + sm.n_short, sm.n_short, sm.n_long, pb.d_smax.get(), pb.d_smax.get() + sm.n_long, nullptr};
            if (y_f64) softmax_bwd_launch<double, double>(c, w, yh, dy64, scale, nullptr, dsh);
            else softmax_bwd_launch<float, double>(c, w, yh, dy64, scale, nullptr, dsh);
            if (want_dq) {
                const PropSide sd{row_ptr, nq, c->sp.d_ids.get(), nullptr, nullptr, false, dsh, true, nullptr};
                const PropGeom gm = prop_geom((uint64_t)(uintptr_t)kh, ldk, d, k_elt, widths_k, PROP_NWIDTHS);
                prop_launch_chunks(c, plan.lng, segs, pb.d_recs.get(), sd, k_type, gm, kh, ldk, d, nullptr, dq32.ptr((uint64_t)h * d), dq32.ld(), dq64.ptr((uint64_t)h * d), dq64.ld(), false);
            }
        }
        if (want_dk) if (int rc = attn_bwd_cols(c, heads, entries, ds, true, q.ptr(), q_type, ldq, d, dk32.ptr(), dk32.ld(), dk64.ptr(), dk64.ld())) return rc;
        if (want_dv) if (int rc = attn_bwd_cols(c, heads, entries, y.ptr(), y_f64, g.ptr(), g_type, ldg, dv, dv32.ptr(), dv32.ld(), dv64.ptr(), dv64.ld())) return rc;
    }
    if (int rc = held_fetch(c, dq32, dq64, dk32, dk64, dv32, dv64)) return rc;
    if (int rc = held_call_end(c, "sparse attention_bwd")) return rc;
    if (st) {
        st->entries = entries; st->segments = plan.segments; st->max_row = plan.max_row;
        st->short_rows = plan.short_rows; st->long_rows = plan.long_rows;
        if (want_cols) {
            const AttnColPlan &cp = t.cols.plan;
            st->columns = cp.columns; st->max_col = cp.max_col; st->short_cols = cp.short_cols; st->long_cols = cp.long_cols;
        }
        st->built = built_now ? 1 : 0; st->plan_cached = plan_cached ? 1 : 0;
        st->q_on_device = q.on_device(); st->k_on_device = k.on_device(); st->v_on_device = v.on_device(); st->g_on_device = g.on_device();
        st->y_on_device = y.on_device();
        st->transpose_ms = built_now ? c->tm.propt_transpose_ms : 0.0; st->attn_ms = c->tm.attn_ms;
    }
    return FORA_OK;
}
} // namespace

// =============================================================================== C ABI
extern "C" {

int fora_hip_device_count(void) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return 0;
    return ndev;
}

int fora_hip_create(int device, fora_ctx **out) {
    if (!out) return FORA_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return FORA_E_NOGPU;
    if (device < 0 || device >= ndev) return FORA_E_ARG;
    fora_ctx *c = new (std::nothrow) fora_ctx();
    if (!c) return FORA_E_NOMEM;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&c->prop, device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return FORA_E_HIP;
    }
    if (strncmp(c->prop.gcnArchName, "gfx950", 6) != 0) {
        // kernels are compiled for gfx950 only
        (void)hipStreamDestroy(c->stream);
        delete c;
        return FORA_E_NOGPU;
    }
    if (c->d_stamps.alloc(32) != hipSuccess || hipMemset(c->d_stamps.get(), 0, 32 * sizeof(unsigned long long)) != hipSuccess) {
        c->d_stamps.reset();
        (void)hipStreamDestroy(c->stream);
        delete c;
        return FORA_E_NOMEM;
    }
    c->opt_ = tunables_from_env();
    apply_options(c);
    *out = c;
    return FORA_OK;
}

void fora_hip_destroy(fora_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_workspace(c);
    free_index(c);
    free_graph(c);
    free_sparse(c);
    free_sweep(c);
    free_prop(c);
    free_store(c);
    free_cols(c);
    free_sub(c);
    c->bw = BwdBufs{};
    c->d_stamps.reset();
    for (auto &p : c->tm.ev_pool) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *fora_hip_last_error(fora_ctx *c) { return c ? c->err.c_str() : "null ctx"; }

int fora_hip_device_info(fora_ctx *c, char *arch, int arch_len, int *cus, uint64_t *hbm_bytes) {
    if (!c) return FORA_E_ARG;
    if (arch && arch_len > 0) { strncpy(arch, c->prop.gcnArchName, (size_t)arch_len - 1); arch[arch_len - 1] = 0; }
    if (cus) *cus = c->prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (uint64_t)c->prop.totalGlobalMem;
    return FORA_OK;
}


int fora_hip_set_graph(fora_ctx *c, int32_t n, int64_t m_attr, const int64_t *row_ptr, const int32_t *col) {
    if (!c) return FORA_E_ARG;
    if (n <= 0 || !row_ptr || row_ptr[0] != 0) return fail(c, FORA_E_ARG, "bad graph");
    const int64_t nnz = row_ptr[n];
    if (nnz < 0 || (nnz && !col) || nnz >= (1ll << 32)) return fail(c, FORA_E_ARG, "bad graph (nnz): at most 2^32 - 1 edges");
    for (int32_t v = 0; v < n; v++)
        if (row_ptr[v + 1] < row_ptr[v]) return fail(c, FORA_E_ARG, "row_ptr not monotone");
    for (int64_t e = 0; e < nnz; e++)
        if (col[e] < 0 || col[e] >= n) return fail(c, FORA_E_ARG, "edge target out of range"); // graph.h:155-156
    HIPCHK(c, hipSetDevice(c->device));
    free_workspace(c);
    free_index(c);
    free_graph(c);
    free_sparse(c); // (rows of another graph)
    free_sweep(c);
    free_prop(c); // (the upload of another graph's features)
    free_store(c); // (rows over another graph's nodes)
    free_cols(c); // (a bitmap over another graph's nodes)
    free_sub(c); // (edges of another graph)
    c->sd = SeedBufs{}; // (a block sized for another n; until here it holds ns * n * 8 bytes that later calls cannot plan slots in)
    c->retry.scale = 1; c->retry.scale_topk = 1;
    const int rc = [&]() -> int {
        const RowBasics rb = make_row_basics(n, row_ptr);
        if (!rb.ok) return fail(c, FORA_E_ARG, "out-degree over 2^32");
        HIPCHK(c, c->g.d_row_ptr.upload(row_ptr, (size_t)n + 1));
        HIPCHK(c, c->g.d_col.upload(col, (size_t)nnz, 1));
        HIPCHK(c, c->g.d_rowinfo.upload(rb.rowinfo));
        HIPCHK(c, c->g.d_deg.upload(rb.deg));
        if (nnz < (1ll << 31) && c->opt_.no_compact != 1) { // compact walk-step copy
            const CompactWalk w = make_compact_walk(n, row_ptr, col);
            HIPCHK(c, c->g.d_rp32.upload(w.rp32));
            HIPCHK(c, c->g.d_colp.upload(w.colp));
            c->g.colbits = w.bits;
        }
        c->g.h_row_ptr.assign(row_ptr, row_ptr + n + 1);
        c->g.n = n; c->g.m_attr = m_attr; c->g.nnz = nnz;
        c->g.dangling_frac = (double)rb.n_dangling / (double)n;
        if (int rw = build_walk_dg(c, row_ptr, col)) return rw;
        if (int rt = ensure_team(c)) return rt; // (before the hub copy: its size depends on whether the team path takes this graph)
        if (int rh = build_hub_copy(c, col)) return rh;
        return build_quad_copies(c);
    }();
    if (rc) free_graph(c); // no half-built graph: the next call answers "set_graph first"
    return rc;
}

int fora_hip_set_params(fora_ctx *c, double alpha, double epsilon, double rmax_scale, int opt, uint64_t seed) {
    if (!c) return FORA_E_ARG;
    if (!c->g.n) return fail(c, FORA_E_ARG, "set_graph first");
    if (!(alpha > 0 && alpha < 1) || !(epsilon > 0) || !(rmax_scale >= 0)) return fail(c, FORA_E_ARG, "bad params");
    // graph.h:177-178 then algo.h:455-463, in the reference's operand order
    const double delta = 1.0 / c->g.n, pfail = 1.0 / c->g.n;
    const long long m = c->g.m_attr;
    double rmax = epsilon * sqrt(delta / 3 / m / log(2 / pfail));
    if (opt) rmax *= rmax_scale / (1 - alpha);
    else rmax *= rmax_scale;
    const double omega = (2 + epsilon) * log(2 / pfail) / delta / epsilon / epsilon;
    c->par = Params{true, alpha, epsilon, rmax_scale, rmax, omega, opt ? 1 : 0, seed};
    return FORA_OK;
}

int fora_hip_set_params_raw(fora_ctx *c, double alpha, double rmax, double omega, int opt, uint64_t seed) {
    if (!c) return FORA_E_ARG;
    if (!(alpha > 0 && alpha < 1) || !(rmax > 0) || !(omega >= 0)) return fail(c, FORA_E_ARG, "bad params");
    c->par.alpha = alpha; c->par.rmax = rmax; c->par.omega = omega; c->par.opt = opt ? 1 : 0; c->par.seed = seed;
    c->par.have = true;
    return FORA_OK;
}

int fora_hip_get_params(fora_ctx *c, double *rmax, double *omega) {
    if (!c || !c->par.have) return FORA_E_ARG;
    if (rmax) *rmax = c->par.rmax;
    if (omega) *omega = c->par.omega;
    return FORA_OK;
}

int fora_hip_set_batch(fora_ctx *c, int batch) {
    if (!c || batch < 0) return FORA_E_ARG;
    if (batch != c->batch_req) { (void)hipSetDevice(c->device); free_workspace(c); }
    c->batch_req = batch;
    return FORA_OK;
}
int fora_hip_get_batch(fora_ctx *c) { return c ? c->ws.B : FORA_E_ARG; }

int fora_hip_set_option(fora_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return FORA_E_ARG;
    if (!strcmp(name, "reset")) { // back to the defaults / environment of fora_hip_create
        (void)hipSetDevice(c->device);
        free_workspace(c);
        c->opt_ = tunables_from_env();
        c->pt = PropTBufs{}; // (built under another "propt_lds_cap", for all we know)
        c->team_run.suspend = 0; // (a time-out's back-off too)
        apply_options(c);
        return FORA_OK;
    }
    if (!TEST_PATHS && schedule_option(name) && value != (strcmp(name, "rounds") ? (strcmp(name, "round_div") ? 0 : 4) : 1))
        return fail(c, FORA_E_ARG, std::string("option ") + name + ": the schedule experiments are not compiled into this library (build with -DFORA_TEST_PATHS=1: libfora_hip_test.so)");
    for (const auto &o : OPTIONS)
        if (!strcmp(name, o.name)) {
            if (c->opt_.*(o.field) == value) return FORA_OK;
            c->opt_.*(o.field) = value;
            if (o.layout) { (void)hipSetDevice(c->device); free_workspace(c); }
            if (o.field == &Tunables::propt_lds_cap) { (void)hipSetDevice(c->device); c->pt = PropTBufs{}; } // the next transposed call builds again, on the new tiers
            apply_options(c);
            return FORA_OK;
        }
    return fail(c, FORA_E_ARG, std::string("unknown option ") + name);
}

int fora_hip_get_option(fora_ctx *c, const char *name, int64_t *value) {
    if (!name || !value) return FORA_E_ARG;
    // properties of the BUILD: answered without a context (and so without a GPU)
    if (!strcmp(name, "test_paths")) { *value = TEST_PATHS ? 1 : 0; return FORA_OK; } // 1: libfora_hip_test.so (schedule experiments compiled in)
    if (!strcmp(name, "diag_build")) { *value = FORA_DIAG_BUILD; return FORA_OK; }    // 1: a probe / stamp / fake build (fora_diag.h) -- never the shipped library
    if (!c) return FORA_E_ARG;
    // read-only state of the engine beside the knobs
    if (!strcmp(name, "bucket_retries")) { *value = (int64_t)c->retry.retries; return FORA_OK; } // re-runs with doubled message buckets
    if (!strcmp(name, "team_fallbacks")) { *value = (int64_t)c->team_run.fallbacks; return FORA_OK; } // calls re-run with the bucketed push after a team time-out
    if (!strcmp(name, "team_suspended")) { *value = c->team_run.suspend; return FORA_OK; }             // calls left that do not try the team push
    if (!strcmp(name, "sparse_generation")) { *value = (int64_t)c->sparse_gen; return FORA_OK; }    // moves whenever a sparse result becomes held or stops being held
    if (!strcmp(name, "sparse_cols")) { *value = (int64_t)held_cols(c); return FORA_OK; }           // the columns of the calls on the held rows: n, or nc while a compacted result is held (COLUMNS)
    if (!strcmp(name, "sub_edges")) { *value = c->sp.valid && c->sp.compacted && c->sb.valid ? (int64_t)c->sb.edges : -1; return FORA_OK; } // the edges of the held subgraph (SUBGRAPH); -1: none is held
    if (!strcmp(name, "team_members")) { *value = c->g.team.T; return FORA_OK; }                      // 0: this graph / workspace has no team push
    if (!strcmp(name, "team_local_ids")) { *value = c->g.team.T ? c->g.team.R : 0; return FORA_OK; }   // R of the built team tables: local ids per member (0: no team push)
    if (!strcmp(name, "team_hub_sums")) { *value = c->g.team.T ? c->g.team.H : 0; return FORA_OK; }    // their H: hub sums per member, after the cut to the free LDS (0: none, or no team push)
    if (!strcmp(name, "walk_dg_wgs_per_cu")) { // k_walk_dg's resident workgroups per CU at this graph's tables (0: the graph has no degree-grouped copy)
        const WalkDG &g = c->g.walk.dg;
        int wgs = 0;
        if (g.colp) {
            const bool xl = c->opt_.walk_dg != 1 && g.invb;
            (void)hipSetDevice(c->device);
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, (const void *)walk_dg_kernel(false, g.bits32 != 0, xl, walk_flush_align(c)), DG_THREADS, walk_dg_lds(g, xl)) != hipSuccess)
                return fail(c, FORA_E_HIP, "hipOccupancyMaxActiveBlocksPerMultiprocessor(k_walk_dg)");
        }
        *value = wgs;
        return FORA_OK;
    }
    if (!strcmp(name, "team_cooperative")) { *value = c->team_run.coop_ok && !c->team_run.coop_failed ? 1 : 0; return FORA_OK; }
    for (const auto &o : OPTIONS)
        if (!strcmp(name, o.name)) { *value = c->opt_.*(o.field); return FORA_OK; }
    return fail(c, FORA_E_ARG, std::string("unknown option ") + name);
}

int fora_hip_set_balanced(fora_ctx *c, int on, double start_scale, double c_pop, double c_edge, double t_walk, double t_idx) {
    if (!c) return FORA_E_ARG;
    const Balanced def; // (the defaults: its initialisers)
    c->bal.on = on != 0;
    c->bal.start = start_scale > 0 ? start_scale : def.start;
    c->bal.c_pop = c_pop > 0 ? c_pop : def.c_pop;
    c->bal.c_edge = c_edge > 0 ? c_edge : def.c_edge;
    c->bal.t_walk = t_walk > 0 ? t_walk : def.t_walk;
    c->bal.t_idx = t_idx > 0 ? t_idx : def.t_idx;
    return FORA_OK;
}

// ---- index ---------------------------------------------------------------------
static uint64_t host_index_sizes(const fora_ctx *c, uint64_t *off, uint64_t *cnt) {
    // build.h:325-334
    uint64_t total = 0;
    for (int32_t v = 0; v < c->g.n; v++) {
        const size_t deg = (size_t)(c->g.h_row_ptr[v + 1] - c->g.h_row_ptr[v]);
        unsigned long num_rw;
        if (c->par.opt) num_rw = (unsigned long)ceil(deg * c->par.rmax * (1 - c->par.alpha) * c->par.omega);
        else num_rw = (unsigned long)ceil(deg * c->par.rmax * c->par.omega);
        if (off) off[v] = total;
        if (cnt) cnt[v] = num_rw;
        total += num_rw;
    }
    return total;
}

int fora_hip_index_sizes(fora_ctx *c, uint64_t *total, uint64_t *off, uint64_t *cnt) {
    if (!c || !c->g.n || !c->par.have) return fail(c, FORA_E_ARG, "set_graph and set_params first");
    const uint64_t t = host_index_sizes(c, off, cnt);
    if (total) *total = t;
    return FORA_OK;
}

int fora_hip_build_index(fora_ctx *c) {
    if (!c || !c->g.n || !c->par.have) return fail(c, FORA_E_ARG, "set_graph and set_params first");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint64_t> off((size_t)c->g.n), cnt((size_t)c->g.n);
    const uint64_t total = host_index_sizes(c, off.data(), cnt.data());
    free_index(c);
    Index ix;
    HIPCHK(c, ix.d_rw_idx.alloc(std::max<uint64_t>(1, total)));
    HIPCHK(c, ix.d_idx_off.alloc((size_t)c->g.n));
    HIPCHK(c, ix.d_idx_cnt.alloc((size_t)c->g.n));
    HIPCHK(c, hipMemcpy(ix.d_idx_off.get(), off.data(), (size_t)c->g.n * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(ix.d_idx_cnt.get(), cnt.data(), (size_t)c->g.n * 8, hipMemcpyHostToDevice));
    ix.len = total;
    c->retry.div = 1;
    int rc = ensure_workspace(c, 1, (double)total);
    if (rc) return rc;
    Dev d = make_dev(c, 1, false);
    d.rw_idx = ix.d_rw_idx.get(); d.idx_off = ix.d_idx_off.get(); d.idx_cnt = ix.d_idx_cnt.get(); // the index being built
    HIPCHK(c, c->ws.d_counters.zero(c->stream));
    HIPCHK(c, c->ws.d_err.zero(c->stream));
    HIPCHK(c, c->ws.d_wit_count.zero(c->stream));
    const uint32_t chunks = (uint32_t)std::min<int64_t>(((int64_t)c->g.n + BLOCK - 1) / BLOCK, 2048);
    EvSpan ev(c, EV_OTHER);
    hipLaunchKernelGGL(k_index_alloc, dim3(chunks), dim3(BLOCK), 0, c->stream, d);
    ev.begin(EV_WALK);
    hipLaunchKernelGGL(k_walk_online<WALK_TO_INDEX>, dim3(walk_grid_x(c, 1), 1), dim3(BLOCK), 0, c->stream, d, 0u,
                       c->par.opt ? 1 : 0, ix.d_rw_idx.get());
    ev.end();
    if ((rc = close_batch(c, nullptr, "build_index"))) return drop_pairs_unless_ok(c, rc);
    ix.have = true;
    c->ix = std::move(ix);
    return FORA_OK;
}

int fora_hip_get_index(fora_ctx *c, int32_t *rw_idx, uint64_t len, uint64_t *off, uint64_t *cnt) {
    if (!c || !c->ix.have) return fail(c, FORA_E_ARG, "no index");
    if (rw_idx && len < c->ix.len) return fail(c, FORA_E_ARG, "rw_idx buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    if (rw_idx && c->ix.len) HIPCHK(c, hipMemcpy(rw_idx, c->ix.d_rw_idx.get(), c->ix.len * 4, hipMemcpyDeviceToHost));
    if (off) HIPCHK(c, hipMemcpy(off, c->ix.d_idx_off.get(), (size_t)c->g.n * 8, hipMemcpyDeviceToHost));
    if (cnt) HIPCHK(c, hipMemcpy(cnt, c->ix.d_idx_cnt.get(), (size_t)c->g.n * 8, hipMemcpyDeviceToHost));
    return FORA_OK;
}

int fora_hip_set_index(fora_ctx *c, const int32_t *rw_idx, uint64_t len, const uint64_t *off, const uint64_t *cnt) {
    if (!c || !c->g.n) return fail(c, FORA_E_ARG, "set_graph first");
    if (!off || !cnt || (len && !rw_idx)) return fail(c, FORA_E_ARG, "bad index");
    for (int32_t v = 0; v < c->g.n; v++)
        if (off[v] + cnt[v] > len) return fail(c, FORA_E_ARG, "index entry range out of bounds");
    for (uint64_t i = 0; i < len; i++)
        if (rw_idx[i] < 0 || rw_idx[i] >= c->g.n) return fail(c, FORA_E_ARG, "index endpoint out of range");
    HIPCHK(c, hipSetDevice(c->device));
    free_index(c);
    Index ix;
    HIPCHK(c, ix.d_rw_idx.alloc(std::max<uint64_t>(1, len)));
    HIPCHK(c, ix.d_idx_off.alloc((size_t)c->g.n));
    HIPCHK(c, ix.d_idx_cnt.alloc((size_t)c->g.n));
    if (len) HIPCHK(c, hipMemcpy(ix.d_rw_idx.get(), rw_idx, len * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(ix.d_idx_off.get(), off, (size_t)c->g.n * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(ix.d_idx_cnt.get(), cnt, (size_t)c->g.n * 8, hipMemcpyHostToDevice));
    ix.len = len;
    ix.have = true;
    c->ix = std::move(ix);
    return FORA_OK;
}

int fora_hip_clear_index(fora_ctx *c) {
    if (!c) return FORA_E_ARG;
    (void)hipSetDevice(c->device);
    free_index(c);
    return FORA_OK;
}

// ---- queries -------------------------------------------------------------------
int fora_hip_query_batch(fora_ctx *c, const int32_t *sources, int nq, int with_idx, double *ppr_out,
                         fora_query_stats *stats) {
    return with_bucket_retry(c, [&] { return query_common(c, sources, nq, with_idx, 0, ppr_out, nullptr, nullptr, stats); });
}

int fora_hip_query_batch_fix(fora_ctx *c, const int32_t *sources, int nq, int with_idx, uint64_t *ppr_fix_out,
                             uint64_t *residue_fix_out, fora_query_stats *stats) {
    return with_bucket_retry(c, [&] { return query_common(c, sources, nq, with_idx, 0, nullptr, ppr_fix_out, residue_fix_out, stats); });
}

// k null: the plain call; otherwise the top-k call with *k
static int query_sparse_call(fora_ctx *c, const int32_t *sources, int nq, int with_idx, double threshold, const int64_t *k, int64_t *row_ptr,
                             fora_query_stats *stats, fora_sparse_stats *sp_out, fora_topk_stats *tk_out) {
    if (!c) return FORA_E_ARG;
    uint64_t thr;
    if (int rc = held_rows_begin(c, c->sp, row_ptr, threshold, thr, k)) return rc;
    return with_bucket_retry(c, [&] {
        SparseRun run; // (a retried attempt starts from an empty one)
        run.thr = thr; run.topk = k ? *k : 0;
        c->tm.sp_compact_ms = c->tm.tk_select_ms = 0;
        if (int rc = query_common(c, sources, nq, with_idx, 0, nullptr, nullptr, nullptr, stats, 0, nullptr, nullptr, &run)) return rc;
        return sparse_finish(c, run, row_ptr, sp_out, tk_out);
    });
}
int fora_hip_query_sparse_batch(fora_ctx *c, const int32_t *sources, int nq, int with_idx, double threshold, int64_t *row_ptr,
                                fora_query_stats *stats, fora_sparse_stats *sp_out) {
    return query_sparse_call(c, sources, nq, with_idx, threshold, nullptr, row_ptr, stats, sp_out, nullptr);
}
// ---- the k largest entries of every sparse row (the SPARSE RESULTS, TOP-K contract of include/fora_hip.h)
int fora_hip_query_sparse_topk_batch(fora_ctx *c, const int32_t *sources, int nq, int with_idx, double threshold, int64_t k, int64_t *row_ptr,
                                     fora_query_stats *stats, fora_sparse_stats *sp_out, fora_topk_stats *tk_out) {
    return query_sparse_call(c, sources, nq, with_idx, threshold, &k, row_ptr, stats, sp_out, tk_out);
}

// ---- seed sets: weighted multi-seed queries, one row per set (the SEED SETS contract of include/fora_hip.h)
int fora_hip_query_seeds_batch(fora_ctx *c, const int64_t *set_ptr, const int32_t *seeds, const double *weights, int ns, int with_idx,
                               double *ppr_out, uint64_t *ppr_fix_out, int k, int32_t *ids, double *scores, uint64_t *row_sum_fix_out,
                               fora_seeds_stats *st) {
    return with_bucket_retry(c, [&] {
        return query_seeds_impl(c, set_ptr, seeds, weights, ns, with_idx, ppr_out, ppr_fix_out, k, ids, scores, row_sum_fix_out, st);
    });
}

// ---- seed sets, result kept sparse: the set rows thresholded after the sum, held and fetched like fora_hip_query_sparse_batch's
static int seeds_sparse_call(fora_ctx *c, const int64_t *set_ptr, const int32_t *seeds, const double *weights, int ns, int with_idx,
                             double threshold, const int64_t *k, int64_t *row_ptr, uint64_t *row_sum_fix_out, fora_seeds_stats *st,
                             fora_sparse_stats *sp_out, fora_topk_stats *tk_out) {
    if (!c) return FORA_E_ARG;
    uint64_t thr;
    if (int rc = held_rows_begin(c, c->sp, row_ptr, threshold, thr, k)) return rc;
    return with_bucket_retry(c, [&] {
        return seeds_sparse_impl(c, set_ptr, seeds, weights, ns, with_idx, thr, row_ptr, row_sum_fix_out, st, sp_out, k ? *k : 0, tk_out);
    });
}
int fora_hip_seeds_sparse_batch(fora_ctx *c, const int64_t *set_ptr, const int32_t *seeds, const double *weights, int ns, int with_idx,
                                double threshold, int64_t *row_ptr, uint64_t *row_sum_fix_out, fora_seeds_stats *st, fora_sparse_stats *sp_out) {
    return seeds_sparse_call(c, set_ptr, seeds, weights, ns, with_idx, threshold, nullptr, row_ptr, row_sum_fix_out, st, sp_out, nullptr);
}
int fora_hip_seeds_sparse_topk_batch(fora_ctx *c, const int64_t *set_ptr, const int32_t *seeds, const double *weights, int ns, int with_idx,
                                     double threshold, int64_t k, int64_t *row_ptr, uint64_t *row_sum_fix_out, fora_seeds_stats *st,
                                     fora_sparse_stats *sp_out, fora_topk_stats *tk_out) {
    return seeds_sparse_call(c, set_ptr, seeds, weights, ns, with_idx, threshold, &k, row_ptr, row_sum_fix_out, st, sp_out, tk_out);
}

// ---- seed sets, swept: the SWEEP CUT contract over the set rows, held and fetched like fora_hip_sweep_batch's
int fora_hip_seeds_sweep_batch(fora_ctx *c, const int64_t *set_ptr, const int32_t *seeds, const double *weights, int ns, int with_idx,
                               double threshold, int64_t max_size, int64_t *row_ptr, fora_sweep_row *rows, fora_seeds_stats *st,
                               fora_sweep_stats *sw_out) {
    if (!c) return FORA_E_ARG;
    uint64_t thr;
    if (int rc = held_rows_begin(c, c->swp, row_ptr, threshold, thr)) return rc;
    return with_bucket_retry(c, [&] {
        return seeds_sweep_impl(c, set_ptr, seeds, weights, ns, with_idx, thr, max_size, row_ptr, rows, st, sw_out);
    });
}

int fora_hip_sparse_fetch(fora_ctx *c, int32_t *ids, double *vals, uint64_t *fix, uint64_t cap) {
    if (!c) return FORA_E_ARG;
    if (!c->sp.valid) return fail(c, FORA_E_ARG, "no sparse result is held");
    if (cap < c->sp.entries) return fail(c, FORA_E_ARG, "cap is smaller than the held result");
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t e = c->sp.entries;
    bool vals_on_device = false;
    if (vals) if (int rc = sparse_dest(c, vals, vals_on_device)) return rc;
    if (e && ids) HIPCHK(c, hipMemcpyAsync(ids, c->sp.d_ids.get(), e * 4, hipMemcpyDefault, c->stream));
    if (e && fix) HIPCHK(c, hipMemcpyAsync(fix, c->sp.d_fix.get(), e * 8, hipMemcpyDefault, c->stream));
    if (e && vals) if (int rc = fetch_vals(c, c->sp.d_fix.get(), e, vals, vals_on_device)) return rc;
    return held_call_end(c, "sparse fetch", false);
}

// ---- PROPAGATE (the contract of include/fora_hip.h): the held sparse rows times a feature matrix, every bit defined
static_assert(PROP_SEG == FORA_PROP_SEG, "fora_prop_plan.h and include/fora_hip.h name one segment length");

// the frame of fora_hip_sparse_propagate and fora_hip_sparse_propagate_vals (with_values: values / val_type are the caller's)
static int prop_entry(fora_ctx *c, const int64_t *row_ptr, int nq, const void *feat, int feat_type, int d, int64_t ldf, int flags, bool with_values,
                      const void *values, int val_type, float *out32, double *out64, int64_t ldo, fora_prop_stats *ps) {
    if (int rc = held_call_begin(c, "sparse propagate", row_ptr, nq)) return rc;
    if (!elt_known(feat_type)) return fail(c, FORA_E_ARG, "sparse propagate: unknown feat_type");
    if (flags & ~FORA_PROP_NORMALIZE) return fail(c, FORA_E_ARG, "sparse propagate: unknown flag");
    if (d < 1 || d > 65536) return fail(c, FORA_E_ARG, "sparse propagate: d outside 1 .. 65536");
    if (ldf < d || ldo < d) return fail(c, FORA_E_ARG, "sparse propagate: a leading dimension smaller than d");
    if (!out32 && !out64) return fail(c, FORA_E_ARG, "sparse propagate: no output");
    if (c->sp.entries && !feat) return fail(c, FORA_E_ARG, "sparse propagate: null feat");
    if (with_values) {
        if (flags & FORA_PROP_NORMALIZE) return fail(c, FORA_E_ARG, "sparse propagate: FORA_PROP_NORMALIZE with values");
        if (val_type != FORA_PROP_F32 && val_type != FORA_PROP_F64) return fail(c, FORA_E_ARG, "sparse propagate: val_type is neither f32 nor f64");
        if (c->sp.entries && !values) return fail(c, FORA_E_ARG, "sparse propagate: null values");
    }
    if (ps) memset(ps, 0, sizeof(*ps));
    if (nq == 0) return FORA_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return drop_pairs_unless_ok(c, prop_impl(c, row_ptr, nq, feat, feat_type, d, ldf, flags, c->sp.entries ? values : nullptr, val_type, out32, out64, ldo, ps));
}
int fora_hip_sparse_propagate(fora_ctx *c, const int64_t *row_ptr, int nq, const void *feat, int feat_type, int d, int64_t ldf, int flags,
                              float *out32, double *out64, int64_t ldo, fora_prop_stats *ps) {
    return prop_entry(c, row_ptr, nq, feat, feat_type, d, ldf, flags, false, nullptr, FORA_PROP_F32, out32, out64, ldo, ps);
}
// ---- PROPAGATE WITH VALUES (the contract of include/fora_hip.h): the same product, the caller's values as the weights
int fora_hip_sparse_propagate_vals(fora_ctx *c, const int64_t *row_ptr, int nq, const void *feat, int feat_type, int d, int64_t ldf, int flags,
                                   const void *values, int val_type, float *out32, double *out64, int64_t ldo, fora_prop_stats *ps) {
    return prop_entry(c, row_ptr, nq, feat, feat_type, d, ldf, flags, true, values, val_type, out32, out64, ldo, ps);
}

// ---- PROPAGATE, TRANSPOSED (the contract of include/fora_hip.h): out = (held rows)^T * grad, n x d, the same fixed order
static int propt_entry(fora_ctx *c, const int64_t *row_ptr, int nq, const void *grad, int grad_type, int d, int64_t ldg, int flags, bool with_values,
                       const void *values, int val_type, float *out32, double *out64, int64_t ldo, fora_propt_stats *ps) {
    if (int rc = held_call_begin(c, "sparse propagate_t", row_ptr, nq)) return rc;
    if (!elt_known(grad_type)) return fail(c, FORA_E_ARG, "sparse propagate_t: unknown grad_type");
    if (flags & ~FORA_PROP_NORMALIZE) return fail(c, FORA_E_ARG, "sparse propagate_t: unknown flag");
    if (d < 1 || d > 65536) return fail(c, FORA_E_ARG, "sparse propagate_t: d outside 1 .. 65536");
    if (ldg < d || ldo < d) return fail(c, FORA_E_ARG, "sparse propagate_t: a leading dimension smaller than d");
    if (!out32 && !out64) return fail(c, FORA_E_ARG, "sparse propagate_t: no output");
    if (c->sp.entries && !grad) return fail(c, FORA_E_ARG, "sparse propagate_t: null grad");
    if (with_values) {
        if (flags & FORA_PROP_NORMALIZE) return fail(c, FORA_E_ARG, "sparse propagate_t: FORA_PROP_NORMALIZE with values");
        if (val_type != FORA_PROP_F32 && val_type != FORA_PROP_F64) return fail(c, FORA_E_ARG, "sparse propagate_t: val_type is neither f32 nor f64");
        if (c->sp.entries && !values) return fail(c, FORA_E_ARG, "sparse propagate_t: null values");
    }
    if (ps) memset(ps, 0, sizeof(*ps));
    HIPCHK(c, hipSetDevice(c->device));
    return drop_pairs_unless_ok(c, propt_impl(c, row_ptr, nq, grad, grad_type, d, ldg, flags, c->sp.entries ? values : nullptr, val_type, out32, out64, ldo, ps));
}
int fora_hip_sparse_propagate_t(fora_ctx *c, const int64_t *row_ptr, int nq, const void *grad, int grad_type, int d, int64_t ldg, int flags,
                                float *out32, double *out64, int64_t ldo, fora_propt_stats *ps) {
    return propt_entry(c, row_ptr, nq, grad, grad_type, d, ldg, flags, false, nullptr, FORA_PROP_F32, out32, out64, ldo, ps);
}
int fora_hip_sparse_propagate_t_vals(fora_ctx *c, const int64_t *row_ptr, int nq, const void *grad, int grad_type, int d, int64_t ldg, int flags,
                                     const void *values, int val_type, float *out32, double *out64, int64_t ldo, fora_propt_stats *ps) {
    return propt_entry(c, row_ptr, nq, grad, grad_type, d, ldg, flags, true, values, val_type, out32, out64, ldo, ps);
}

// ---- SCORES (SDDMM) (the contract of include/fora_hip.h): score_e = <a[row_e], b[id_e]> for every held entry, in a fixed order

int fora_hip_sparse_sddmm(fora_ctx *c, const int64_t *row_ptr, int nq, const void *a, int a_type, int64_t lda, const void *b, int b_type, int64_t ldb, int d,
                          float *out32, double *out64, uint64_t cap, fora_sddmm_stats *st) {
    if (int rc = held_call_begin(c, "sparse sddmm", row_ptr, nq)) return rc;
    if (!elt_known(a_type) || !elt_known(b_type))
        return fail(c, FORA_E_ARG, "sparse sddmm: unknown a_type or b_type");
    if (d < 1 || d > 65536) return fail(c, FORA_E_ARG, "sparse sddmm: d outside 1 .. 65536");
    if (lda < d || ldb < d) return fail(c, FORA_E_ARG, "sparse sddmm: a leading dimension smaller than d");
    if (!out32 && !out64) return fail(c, FORA_E_ARG, "sparse sddmm: no output");
    if (cap < c->sp.entries) return fail(c, FORA_E_ARG, "sparse sddmm: cap is smaller than the held result");
    if (c->sp.entries && (!a || !b)) return fail(c, FORA_E_ARG, "sparse sddmm: null a or b");
    if (st) memset(st, 0, sizeof(*st));
    if (nq == 0) return FORA_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return drop_pairs_unless_ok(c, sddmm_impl(c, row_ptr, nq, a, a_type, lda, b, b_type, ldb, d, out32, out64, st));
}

// ---- ROW SOFTMAX (the contract of include/fora_hip.h): softmax inside every held row and its gradient, in a fixed order

int fora_hip_sparse_softmax(fora_ctx *c, const int64_t *row_ptr, int nq, const void *scores, int val_type, double scale,
                            float *out32, double *out64, uint64_t cap, fora_softmax_stats *st) {
    return softmax_entry(c, "sparse softmax", row_ptr, nq, scores, val_type, false, nullptr, FORA_PROP_F32, scale, out32, out64, cap, st);
}
int fora_hip_sparse_softmax_bwd(fora_ctx *c, const int64_t *row_ptr, int nq, const void *y, int y_type, const void *grad, int g_type, double scale,
                                float *out32, double *out64, uint64_t cap, fora_softmax_stats *st) {
    return softmax_entry(c, "sparse softmax_bwd", row_ptr, nq, y, y_type, true, grad, g_type, scale, out32, out64, cap, st);
}

// ---- ATTENTION (the contract of include/fora_hip.h): SCORES, ROW SOFTMAX and PROPAGATE WITH VALUES per head in one call -- the
// rows of at most "attn_short" entries in the fused kernel (fora_attn.h), the longer ones through the three steps' own kernels

int fora_hip_sparse_attention(fora_ctx *c, const int64_t *row_ptr, int nq, const void *q, int q_type, int64_t ldq, const void *k, int k_type, int64_t ldk,
                              const void *v, int v_type, int64_t ldv, int d, int dv, int heads, double scale, float *out32, double *out64, int64_t ldo,
                              float *y32, double *y64, uint64_t ycap, fora_attn_stats *st) {
    if (int rc = held_call_begin(c, "sparse attention", row_ptr, nq)) return rc;
    if (!elt_known(q_type) || !elt_known(k_type) || !elt_known(v_type)) return fail(c, FORA_E_ARG, "sparse attention: unknown q_type, k_type or v_type");
    if (d < 1 || d > 65536 || dv < 1 || dv > 65536) return fail(c, FORA_E_ARG, "sparse attention: d or dv outside 1 .. 65536");
    if (heads < 1 || (int64_t)heads * d > 65536 || (int64_t)heads * dv > 65536) return fail(c, FORA_E_ARG, "sparse attention: heads < 1, or heads * d or heads * dv over 65536");
    if (ldq < (int64_t)heads * d || ldk < (int64_t)heads * d) return fail(c, FORA_E_ARG, "sparse attention: ldq or ldk smaller than heads * d");
    if (ldv < (int64_t)heads * dv || ldo < (int64_t)heads * dv) return fail(c, FORA_E_ARG, "sparse attention: ldv or ldo smaller than heads * dv");
    if (!std::isfinite(scale)) return fail(c, FORA_E_ARG, "sparse attention: scale is not finite");
    if (!out32 && !out64) return fail(c, FORA_E_ARG, "sparse attention: no output");
    if ((y32 || y64) && ycap < (uint64_t)heads * c->sp.entries) return fail(c, FORA_E_ARG, "sparse attention: ycap is smaller than heads * the held entries");
    if (c->sp.entries && (!q || !k || !v)) return fail(c, FORA_E_ARG, "sparse attention: null q, k or v");
    if (st) memset(st, 0, sizeof(*st));
    if (nq == 0) return FORA_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return drop_pairs_unless_ok(c, attention_impl(c, row_ptr, nq, c->sp.entries ? q : nullptr, q_type, ldq, c->sp.entries ? k : nullptr, k_type, ldk,
                                                  c->sp.entries ? v : nullptr, v_type, ldv, d, dv, heads, scale, out32, out64, ldo, y32, y64, st));
}

// ---- ATTENTION, BACKWARD (the contract of include/fora_hip.h): dq, dk and dv of all heads in one call -- the rows and the columns
// of at most "attn_short" entries in the fused kernels (fora_attn_bwd.h), the longer ones through the chained calls' own kernels

int fora_hip_sparse_attention_bwd(fora_ctx *c, const int64_t *row_ptr, int nq, const void *q, int q_type, int64_t ldq, const void *k, int k_type, int64_t ldk,
                                  const void *v, int v_type, int64_t ldv, const void *g, int g_type, int64_t ldg, const void *y, int y_type, uint64_t ycap,
                                  int d, int dv, int heads, double scale, const fora_attn_grads *grads, fora_attn_bwd_stats *st) {
    if (int rc = held_call_begin(c, "sparse attention_bwd", row_ptr, nq)) return rc;
    const char *who = "sparse attention_bwd: ";
    if (!elt_known(q_type) || !elt_known(k_type) || !elt_known(v_type) || !elt_known(g_type)) return fail(c, FORA_E_ARG, std::string(who) + "unknown q_type, k_type, v_type or g_type");
    if (y_type != FORA_PROP_F32 && y_type != FORA_PROP_F64) return fail(c, FORA_E_ARG, std::string(who) + "y_type is neither f32 nor f64");
    if (d < 1 || d > 65536 || dv < 1 || dv > 65536) return fail(c, FORA_E_ARG, std::string(who) + "d or dv outside 1 .. 65536");
    if (heads < 1 || (int64_t)heads * d > 65536 || (int64_t)heads * dv > 65536) return fail(c, FORA_E_ARG, std::string(who) + "heads < 1, or heads * d or heads * dv over 65536");
    if (ldq < (int64_t)heads * d || ldk < (int64_t)heads * d) return fail(c, FORA_E_ARG, std::string(who) + "ldq or ldk smaller than heads * d");
    if (ldv < (int64_t)heads * dv || ldg < (int64_t)heads * dv) return fail(c, FORA_E_ARG, std::string(who) + "ldv or ldg smaller than heads * dv");
    if (!std::isfinite(scale)) return fail(c, FORA_E_ARG, std::string(who) + "scale is not finite");
    if (!grads) return fail(c, FORA_E_ARG, std::string(who) + "no output");
    const bool want_dq = grads->dq32 || grads->dq64, want_dk = grads->dk32 || grads->dk64, want_dv = grads->dv32 || grads->dv64;
    if (!want_dq && !want_dk && !want_dv) return fail(c, FORA_E_ARG, std::string(who) + "no output");
    if ((want_dq && grads->lddq < (int64_t)heads * d) || (want_dk && grads->lddk < (int64_t)heads * d) || (want_dv && grads->lddv < (int64_t)heads * dv))
        return fail(c, FORA_E_ARG, std::string(who) + "lddq or lddk smaller than heads * d, or lddv smaller than heads * dv");
    if (ycap < (uint64_t)heads * c->sp.entries) return fail(c, FORA_E_ARG, std::string(who) + "ycap is smaller than heads * the held entries");
    if (c->sp.entries && (!q || !k || !v || !g || !y)) return fail(c, FORA_E_ARG, std::string(who) + "null q, k, v, g or y");
    if (st) memset(st, 0, sizeof(*st));
    if (nq == 0) return FORA_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const bool e = c->sp.entries != 0;
    return drop_pairs_unless_ok(c, attention_bwd_impl(c, row_ptr, nq, e ? q : nullptr, q_type, ldq, e ? k : nullptr, k_type, ldk, e ? v : nullptr, v_type, ldv,
                                                      e ? g : nullptr, g_type, ldg, e ? y : nullptr, y_type, d, dv, heads, scale, *grads, st));
}

int fora_hip_sparse_transpose_fetch(fora_ctx *c, const int64_t *row_ptr, int nq, int64_t *col_ptr, int32_t *rows, uint64_t *fix, double *vals, uint64_t cap) {
    if (!c) return FORA_E_ARG;
    if (!c->sp.valid) return fail(c, FORA_E_ARG, "no sparse result is held");
    if (nq < 0 || !prop_row_ptr_ok(row_ptr, nq, c->sp.entries)) return fail(c, FORA_E_ARG, "sparse transpose fetch: row_ptr is not the held result's");
    if (cap < c->sp.entries) return fail(c, FORA_E_ARG, "cap is smaller than the held result");
    HIPCHK(c, hipSetDevice(c->device));
    bool dev = false, vals_on_device = false;
    if (col_ptr) if (int rc = sparse_dest(c, col_ptr, dev)) return rc;
    if (rows) if (int rc = sparse_dest(c, rows, dev)) return rc;
    if (fix) if (int rc = sparse_dest(c, fix, dev)) return rc;
    if (vals) if (int rc = sparse_dest(c, vals, vals_on_device)) return rc;
    bool built_now = false;
    if (int rc = drop_pairs_unless_ok(c, propt_ensure(c, row_ptr, nq, built_now))) return rc;
    const PropTBufs &t = c->pt;
    const uint64_t e = c->sp.entries;
    if (col_ptr) HIPCHK(c, hipMemcpyAsync(col_ptr, t.d_col_ptr.get(), ((size_t)held_cols(c) + 1) * 8, hipMemcpyDefault, c->stream));
    if (e && rows) HIPCHK(c, hipMemcpyAsync(rows, t.d_rows.get(), e * 4, hipMemcpyDefault, c->stream));
    if (e && fix) HIPCHK(c, hipMemcpyAsync(fix, t.d_fix.get(), e * 8, hipMemcpyDefault, c->stream));
    if (e && vals) if (int rc = fetch_vals(c, t.d_fix.get(), e, vals, vals_on_device)) return rc;
    return held_call_end(c, "sparse transpose fetch", false);
}

// ---- sweep cut: local clustering over the rows of a query (the SWEEP CUT contract of include/fora_hip.h)
int fora_hip_sweep_batch(fora_ctx *c, const int32_t *sources, int nq, int with_idx, double threshold, int64_t max_size, int64_t *row_ptr,
                         fora_sweep_row *rows, fora_query_stats *stats, fora_sweep_stats *sw_out) {
    if (!c) return FORA_E_ARG;
    uint64_t thr;
    if (int rc = held_rows_begin(c, c->swp, row_ptr, threshold, thr)) return rc;
    return with_bucket_retry(c, [&] {
        SweepRun run(thr, max_size, nq); // (a retried attempt starts from an empty one)
        c->tm.sw_compact_ms = c->tm.sw_sort_ms = c->tm.sw_cut_ms = 0;
        if (int rc = query_common(c, sources, nq, with_idx, 0, nullptr, nullptr, nullptr, stats, 0, nullptr, nullptr, nullptr, &run)) return rc;
        return sweep_finish(c, run, row_ptr, rows, sw_out);
    });
}

int fora_hip_sweep_fetch(fora_ctx *c, int32_t *ids, uint64_t *cut, uint64_t *vol, uint64_t cap) {
    if (!c) return FORA_E_ARG;
    if (!c->swp.valid) return fail(c, FORA_E_ARG, "no sweep result is held");
    if (cap < c->swp.entries) return fail(c, FORA_E_ARG, "cap is smaller than the held result");
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t e = c->swp.entries;
    bool on_device = false;
    for (const void *p : {(const void *)ids, (const void *)cut, (const void *)vol})
        if (p) if (int rc = sparse_dest(c, p, on_device)) return rc;
    if (e && ids) HIPCHK(c, hipMemcpyAsync(ids, c->swp.d_ids.get(), e * 4, hipMemcpyDefault, c->stream));
    if (e && cut) HIPCHK(c, hipMemcpyAsync(cut, c->swp.d_cut.get(), e * 8, hipMemcpyDefault, c->stream));
    if (e && vol) HIPCHK(c, hipMemcpyAsync(vol, c->swp.d_vol.get(), e * 8, hipMemcpyDefault, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FORA_OK;
}

int fora_hip_sweep_clear(fora_ctx *c) {
    if (!c) return FORA_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_sweep(c);
    return FORA_OK;
}

#if FORA_TEST_PATHS
// ---- TEST ENTRY POINTS (include/fora_hip.h; libfora_hip_test.so only): chosen inputs in front of the sweep's own host
// functions and kernels.
// fora_hip_sweep_batch's frame with the caller's rows in the ppr slabs instead of a query batch's: row i takes slot i - b0 of
// its batch, no row is skipped (a RowLayout without sources).
int fora_hip_test_sweep_rows(fora_ctx *c, const uint64_t *rows_fix, int nq, double threshold, int64_t max_size, int64_t *row_ptr,
                             fora_sweep_row *rows, fora_sweep_stats *sw_out) {
    if (!c) return FORA_E_ARG;
    uint64_t thr;
    if (int rc = held_rows_begin(c, c->swp, row_ptr, threshold, thr)) return rc;
    return with_bucket_retry(c, [&] {
        SweepRun run(thr, max_size, nq);
        c->tm.sw_compact_ms = c->tm.sw_sort_ms = c->tm.sw_cut_ms = 0;
        if (int rc = check_batch_args(c, reinterpret_cast<const int32_t *>(rows_fix), nq, "row")) return rc;
        HIPCHK(c, hipSetDevice(c->device));
        const uint64_t n = (uint64_t)c->g.n;
        run.lay.begin(nullptr, nq);
        if (nq) {
            if (int rc = sweep_prepare_rank(c, nq)) return rc;
            if (int rc = ensure_query_workspace(c, nq, 0)) return rc;
            const int per = even_batch(nq, c->ws.B);
            if (int rc = sweep_prepare(c, run, std::min(per, nq))) return rc;
            for (int b0 = 0; b0 < nq; b0 += per) {
                const int nb = std::min(per, nq - b0);
                if ((uint64_t)nb * n > c->ws.d_ppr.size()) return fail(c, FORA_E_HIP, "test_sweep_rows: the batch does not fit the ppr slabs");
                HIPCHK(c, hipMemcpyAsync(c->ws.d_ppr.get(), rows_fix + (uint64_t)b0 * n, (uint64_t)nb * n * 8, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream)); // (pageable source)
                if (int rc = sweep_rows_of_batch(c, run, nullptr, b0, nb)) return rc;
            }
        }
        return sweep_finish(c, run, row_ptr, rows, sw_out);
    });
}

// fora_hip_query_sparse_batch's frame in the same way: the caller's rows in the ppr slabs, counted, placed and held by the
// library's own compaction -- a held sparse result of exactly chosen row lengths.
static int test_sparse_rows_call(fora_ctx *c, const uint64_t *rows_fix, int nq, double threshold, const int64_t *k, int64_t *row_ptr,
                                 fora_sparse_stats *sp_out, fora_topk_stats *tk_out) {
    if (!c) return FORA_E_ARG;
    uint64_t thr;
    if (int rc = held_rows_begin(c, c->sp, row_ptr, threshold, thr, k)) return rc;
    return with_bucket_retry(c, [&] {
        SparseRun run;
        run.thr = thr; run.topk = k ? *k : 0;
        c->tm.sp_compact_ms = c->tm.tk_select_ms = 0;
        if (int rc = check_batch_args(c, reinterpret_cast<const int32_t *>(rows_fix), nq, "row")) return rc;
        HIPCHK(c, hipSetDevice(c->device));
        const uint64_t n = (uint64_t)c->g.n;
        run.lay.begin(nullptr, nq);
        if (nq) {
            if (int rc = ensure_query_workspace(c, nq, 0)) return rc;
            const int per = even_batch(nq, c->ws.B);
            if (int rc = sparse_prepare(c, run, std::min(per, nq), nq)) return rc;
            for (int b0 = 0; b0 < nq; b0 += per) {
                const int nb = std::min(per, nq - b0);
                if ((uint64_t)nb * n > c->ws.d_ppr.size()) return fail(c, FORA_E_HIP, "test_sparse_rows: the batch does not fit the ppr slabs");
                HIPCHK(c, hipMemcpyAsync(c->ws.d_ppr.get(), rows_fix + (uint64_t)b0 * n, (uint64_t)nb * n * 8, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream)); // (pageable source)
                if (int rc = count_rows(c, run, nullptr, nb, c->sp.cnt, EV_SP_COMPACT)) return rc;
                HIPCHK(c, hipStreamSynchronize(c->stream)); // (the counts are back)
                if (int rc = sparse_place(c, run, nullptr, b0, nb)) return rc;
            }
        }
        return sparse_finish(c, run, row_ptr, sp_out, tk_out);
    });
}
int fora_hip_test_sparse_rows(fora_ctx *c, const uint64_t *rows_fix, int nq, double threshold, int64_t *row_ptr, fora_sparse_stats *sp_out) {
    return test_sparse_rows_call(c, rows_fix, nq, threshold, nullptr, row_ptr, sp_out, nullptr);
}
// ... and with the selection behind the compaction: fora_hip_query_sparse_topk_batch's frame over the caller's rows
int fora_hip_test_sparse_topk_rows(fora_ctx *c, const uint64_t *rows_fix, int nq, double threshold, int64_t k, int64_t *row_ptr,
                                   fora_sparse_stats *sp_out, fora_topk_stats *tk_out) {
    return test_sparse_rows_call(c, rows_fix, nq, threshold, &k, row_ptr, sp_out, tk_out);
}

// k_sweep_scan on one row in buffers of this call's own: diff_cut / vol as k_sweep_scatter<true> and k_sweep_cut leave them
int fora_hip_test_sweep_scan(fora_ctx *c, int64_t *diff_cut, uint64_t *vol, int64_t L, uint64_t nnz, uint64_t *out6) {
    if (!c) return FORA_E_ARG;
    if (L < 0 || L > 0x7FFFFFFF || (L && (!diff_cut || !vol)) || !out6) return fail(c, FORA_E_ARG, "test_sweep_scan: bad length or null array");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t len = (size_t)L;
    DevBuf<uint64_t> d_cut, d_vol, d_desc; DevBuf<SweepRowOut> d_out;
    const SweepRowDesc rd{0, 0, (uint32_t)L, 0, (uint32_t)L, 0};
    static_assert(sizeof(SweepRowDesc) % 8 == 0, "uploaded as u64 words");
    HIPCHK(c, d_cut.upload(reinterpret_cast<const uint64_t *>(diff_cut), len, 1));
    HIPCHK(c, d_vol.upload(vol, len, 1));
    HIPCHK(c, d_desc.upload(reinterpret_cast<const uint64_t *>(&rd), sizeof(rd) / 8));
    HIPCHK(c, d_out.alloc(1));
    hipLaunchKernelGGL(k_sweep_scan, dim3(1), dim3(BLOCK), 0, c->stream, (const SweepRowDesc *)d_desc.get(), 0u, d_cut.get(), d_vol.get(), (uint64_t)len, nnz, d_out.get());
    SweepRowOut o;
    HIPCHK(c, hipMemcpyAsync(&o, d_out.get(), sizeof(o), hipMemcpyDeviceToHost, c->stream));
    if (len) HIPCHK(c, hipMemcpyAsync(diff_cut, d_cut.get(), len * 8, hipMemcpyDeviceToHost, c->stream));
    if (len) HIPCHK(c, hipMemcpyAsync(vol, d_vol.get(), len * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, FORA_E_HIP, std::string("test_sweep_scan: ") + hipGetErrorString(e));
    out6[0] = (uint64_t)o.len; out6[1] = (uint64_t)o.best; out6[2] = o.cut; out6[3] = o.vol; out6[4] = o.den; out6[5] = o.edges;
    return FORA_OK;
}

// exp_def (fora_softmax_exp.h) of n host doubles on the device, in buffers of this call's own: the device's bits apart from any softmax
int fora_hip_test_exp(fora_ctx *c, const double *t, int64_t n, double *out) {
    if (!c) return FORA_E_ARG;
    if (n < 0 || n > 0x7FFFFFFF || (n && (!t || !out))) return fail(c, FORA_E_ARG, "test_exp: bad length or null array");
    if (!n) return FORA_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> d_t, d_out;
    HIPCHK(c, d_t.upload(t, (size_t)n));
    HIPCHK(c, d_out.alloc((size_t)n));
    hipLaunchKernelGGL(k_softmax_exp, dim3((unsigned)(((uint64_t)n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, (const double *)d_t.get(), (uint64_t)n, d_out.get());
    HIPCHK(c, hipMemcpyAsync(out, d_out.get(), (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, FORA_E_HIP, std::string("test_exp: ") + hipGetErrorString(e));
    return FORA_OK;
}
#endif // FORA_TEST_PATHS

int fora_hip_sparse_clear(fora_ctx *c) {
    if (!c) return FORA_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_sparse(c);
    return FORA_OK;
}

// ---- COLUMNS (the contract of include/fora_hip.h; kernels in fora_cols.h, the arithmetic in fora_cols_plan.h)
namespace {
int cols_compact_impl(fora_ctx *c, int64_t *ncols_out, fora_cols_stats *st) {
    ColsBufs &b = c->cl;
    const uint64_t entries = c->sp.entries, n = (uint64_t)c->g.n;
    const uint64_t words = cols_words(n);
    const uint32_t block = cols_block(c->opt_.cols_block);
    const uint64_t blocks = cols_blocks(words, block);
    const uint64_t room = std::min(entries, n); // (no more distinct ids than entries, or than nodes)
    unsigned long long nc = 0;
    c->tm.cols_ms = 0;
    if (entries) {
        // ---- every buffer before the first launch: a call that finds no room has changed nothing
        const char *what = "the columns";
        if (int rc = prop_ensure(c, b.d_bitmap, (size_t)words, what)) return rc;
        if (int rc = prop_ensure(c, b.d_wrank, (size_t)words, what)) return rc;
        if (int rc = prop_ensure(c, b.d_btot, 2 * (size_t)blocks, what)) return rc; // totals | offsets
        if (int rc = prop_ensure(c, b.d_cols, (size_t)room, what)) return rc;
        if (int rc = prop_ensure(c, b.d_nc, 1, what)) return rc;
        uint32_t *const tot = b.d_btot.get(), *const off = tot + blocks;
        const auto grid = [](uint64_t units) { return dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>(units, 1), 1u << 16)); }; // (the kernels stride over their work)
        const dim3 flat = grid((entries + BLOCK - 1) / BLOCK);
        EvSpan ev(c, EV_COLS);
        HIPCHK(c, hipMemsetAsync(b.d_bitmap.get(), 0, (size_t)words * 8, c->stream));
        hipLaunchKernelGGL(k_cols_mark, flat, dim3(BLOCK), 0, c->stream, (const int32_t *)c->sp.d_ids.get(), entries, (uint32_t)n, b.d_bitmap.get());
        hipLaunchKernelGGL(k_cols_totals, grid(blocks), dim3(BLOCK), 0, c->stream, (const unsigned long long *)b.d_bitmap.get(), words, block, blocks, tot);
        hipLaunchKernelGGL(k_cols_scan, dim3(1), dim3(BLOCK), 0, c->stream, (const uint32_t *)tot, blocks, off, b.d_nc.get());
        hipLaunchKernelGGL(k_cols_list, grid(blocks), dim3(BLOCK), 0, c->stream, (const unsigned long long *)b.d_bitmap.get(), words, block, blocks, (const uint32_t *)off,
                           b.d_wrank.get(), b.d_cols.get(), room);
        hipLaunchKernelGGL(k_cols_relabel, flat, dim3(BLOCK), 0, c->stream, c->sp.d_ids.get(), entries, (uint32_t)n, (const unsigned long long *)b.d_bitmap.get(),
                           (const uint32_t *)b.d_wrank.get());
        ev.end();
        // (a failure behind the first launch: the ids are neither the old nor the new ones for all we know, nothing stays held)
        if (const hipError_t e = hipMemcpyAsync(&nc, b.d_nc.get(), sizeof(nc), hipMemcpyDeviceToHost, c->stream); e != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            sparse_unheld(c);
            return fail(c, FORA_E_HIP, std::string("sparse compact: ") + hipGetErrorString(e));
        }
    }
    if (int rc = held_call_end(c, "sparse compact")) { sparse_unheld(c); return rc; }
    if (nc > room) { sparse_unheld(c); return fail(c, FORA_E_HIP, "sparse compact: more columns than the held entries or the nodes"); }
    // ---- the held result is over its own columns from here on: the ids changed, so the transposition goes and the generation moves
    c->sp.compacted = true; c->sp.cols = nc;
    c->pt = PropTBufs{};
    c->sparse_gen++;
    *ncols_out = (int64_t)nc;
    if (st) { st->entries = entries; st->cols = nc; st->words = entries ? words : 0; st->cols_ms = c->tm.cols_ms; }
    return FORA_OK;
}
} // namespace

int fora_hip_sparse_compact(fora_ctx *c, const int64_t *row_ptr, int nq, int64_t *ncols_out, fora_cols_stats *st) {
    if (int rc = held_call_begin(c, "sparse compact", row_ptr, nq)) return rc;
    if (!ncols_out) return fail(c, FORA_E_ARG, "sparse compact: ncols_out is required");
    if (c->sp.compacted) return fail(c, FORA_E_ARG, "sparse compact: the held result is compacted already");
    if (st) memset(st, 0, sizeof(*st));
    HIPCHK(c, hipSetDevice(c->device));
    return drop_pairs_unless_ok(c, cols_compact_impl(c, ncols_out, st));
}

int fora_hip_sparse_cols_fetch(fora_ctx *c, int32_t *cols, uint64_t cap) {
    if (!c) return FORA_E_ARG;
    if (!c->sp.valid || !c->sp.compacted) return fail(c, FORA_E_ARG, "sparse cols fetch: no compacted sparse result is held");
    if (cap < c->sp.cols) return fail(c, FORA_E_ARG, "sparse cols fetch: cap is smaller than the held columns");
    if (c->sp.cols && !cols) return fail(c, FORA_E_ARG, "sparse cols fetch: null cols");
    HIPCHK(c, hipSetDevice(c->device));
    bool on_device = false;
    if (cols) if (int rc = sparse_dest(c, cols, on_device)) return rc;
    if (c->sp.cols) HIPCHK(c, hipMemcpyAsync(cols, c->cl.d_cols.get(), c->sp.cols * 4, hipMemcpyDefault, c->stream));
    return held_call_end(c, "sparse cols fetch", false);
}

// ---- SUBGRAPH (the contract of include/fora_hip_ext.h; kernels in fora_subgraph.h, the arithmetic in fora_subgraph_plan.h)
namespace {
// a word of the device on the host, the stream idle behind it; a failure leaves no subgraph held (the call only reads the held result)
int sub_read(fora_ctx *c, const unsigned long long *d, unsigned long long &v) {
    int rc = FORA_OK;
    if (const hipError_t e = hipMemcpyAsync(&v, d, sizeof(v), hipMemcpyDeviceToHost, c->stream); e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        rc = fail(c, FORA_E_HIP, std::string("sparse subgraph: ") + hipGetErrorString(e));
    } else rc = held_call_end(c, "sparse subgraph", false);
    if (rc) c->sb.valid = false;
    return rc;
}
int subgraph_impl(fora_ctx *c, int64_t *edges_out, uint64_t *scanned_out, double *ms_out) {
    SubBufs &b = c->sb;
    const ColsBufs &cl = c->cl;
    const uint64_t nc = c->sp.cols, nnz = (uint64_t)c->g.nnz;
    const uint32_t n = (uint32_t)c->g.n, span = sub_span(c->opt_.sub_span);
    unsigned long long S = 0, edges = 0;
    c->tm.sub_ms = 0;
    sub_prop_drop(c); // (the transposition and the plans of SUBGRAPH PRODUCTS were made from the arrays this call writes again)
    if (nc) {
        // ---- every buffer whose size is known before the first launch: a call that finds no room has changed nothing
        const char *what = "the subgraph";
        const uint64_t rblocks = (nc + BLOCK - 1) / BLOCK;
        if (int rc = prop_ensure(c, b.d_scan, (size_t)nc + 1, what)) return rc;
        if (int rc = prop_ensure(c, b.d_base, (size_t)nc, what)) return rc;
        if (int rc = prop_ensure(c, b.d_rtot, 2 * (size_t)rblocks, what)) return rc; // totals | offsets
        if (int rc = prop_ensure(c, b.d_tot, 2, what)) return rc;                    // S | edges
        if (int rc = prop_ensure(c, b.d_ptr, (size_t)nc + 1, what)) return rc;
        const auto grid = [](uint64_t units) { return dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>(units, 1), 1u << 16)); }; // (the kernels stride over their work)
        const int32_t *U = cl.d_cols.get();
        const int64_t *row_ptr = c->g.d_row_ptr.get();
        const unsigned long long *bitmap = cl.d_bitmap.get();
        uint64_t *const rtot = b.d_rtot.get(), *const roff = rtot + rblocks;
        { // rows: the out-degrees of U, scanned
            EvSpan ev(c, EV_SUB);
            hipLaunchKernelGGL(k_sub_row_totals, grid(rblocks), dim3(BLOCK), 0, c->stream, U, nc, row_ptr, n, rblocks, rtot);
            hipLaunchKernelGGL(k_sub_scan<uint64_t>, dim3(1), dim3(BLOCK), 0, c->stream, (const uint64_t *)rtot, rblocks, roff, b.d_tot.get());
            hipLaunchKernelGGL(k_sub_row_list, grid(rblocks), dim3(BLOCK), 0, c->stream, U, nc, row_ptr, n, rblocks, (const uint64_t *)roff, b.d_scan.get(), b.d_base.get());
        }
        if (int rc = sub_read(c, b.d_tot.get(), S)) return rc; // (the first of the call's two synchronisations: S sizes the spans)
        if (S > nnz) { b.valid = false; return fail(c, FORA_E_HIP, "sparse subgraph: more scanned edges than the graph has"); }
        const uint64_t spans = sub_spans(S, span);
        if (spans) {
            if (int rc = prop_ensure(c, b.d_cnt, (size_t)spans, what)) return rc;
            if (int rc = prop_ensure(c, b.d_off, (size_t)spans, what)) return rc;
            {
                EvSpan ev(c, EV_SUB);
                hipLaunchKernelGGL(k_sub_count, grid(spans), dim3(BLOCK), 0, c->stream, (const int64_t *)b.d_scan.get(), (const int64_t *)b.d_base.get(), nc, (uint64_t)S, span, spans,
                                   (const int32_t *)c->g.d_col.get(), nnz, bitmap, n, b.d_cnt.get());
                hipLaunchKernelGGL(k_sub_scan<uint32_t>, dim3(1), dim3(BLOCK), 0, c->stream, (const uint32_t *)b.d_cnt.get(), spans, b.d_off.get(), b.d_tot.get() + 1);
            }
            if (int rc = sub_read(c, b.d_tot.get() + 1, edges)) return rc; // (the second: the edges size sub_col and sub_eid)
            if (edges > S) { b.valid = false; return fail(c, FORA_E_HIP, "sparse subgraph: more kept edges than scanned ones"); }
            if (int rc = prop_ensure(c, b.d_col, (size_t)edges, what)) return rc;
            if (int rc = prop_ensure(c, b.d_eid, (size_t)edges, what)) return rc;
            b.valid = false; // (sub_ptr, sub_col and sub_eid are written from here on)
            EvSpan ev(c, EV_SUB);
            hipLaunchKernelGGL(k_sub_write, grid(spans), dim3(BLOCK), ((size_t)span + 1) * sizeof(uint32_t), c->stream, (const int64_t *)b.d_scan.get(), (const int64_t *)b.d_base.get(), nc,
                               (uint64_t)S, span, spans, (const int32_t *)c->g.d_col.get(), nnz, bitmap, (const uint32_t *)cl.d_wrank.get(), n, (const uint64_t *)b.d_off.get(),
                               b.d_ptr.get(), b.d_col.get(), b.d_eid.get(), (uint64_t)edges);
        } else { // no node of U has an out-edge: nc + 1 offsets of 0
            b.valid = false;
            if (const hipError_t e = hipMemsetAsync(b.d_ptr.get(), 0, ((size_t)nc + 1) * 8, c->stream); e != hipSuccess) return fail(c, FORA_E_HIP, std::string("sparse subgraph: ") + hipGetErrorString(e));
        }
    }
    if (int rc = held_call_end(c, "sparse subgraph")) { b.valid = false; return rc; }
    b.valid = true; b.edges = edges;
    *edges_out = (int64_t)edges;
    if (scanned_out) *scanned_out = S;
    if (ms_out) *ms_out = c->tm.sub_ms;
    return FORA_OK;
}
} // namespace

int fora_hip_sparse_subgraph(fora_ctx *c, const int64_t *row_ptr, int nq, int64_t *edges_out, uint64_t *scanned_out, double *ms_out) {
    if (int rc = held_call_begin(c, "sparse subgraph", row_ptr, nq)) return rc;
    if (!edges_out) return fail(c, FORA_E_ARG, "sparse subgraph: edges_out is required");
    if (!c->sp.compacted) return fail(c, FORA_E_ARG, "sparse subgraph: the held result is not compacted (fora_hip_sparse_compact first)");
    HIPCHK(c, hipSetDevice(c->device));
    return drop_pairs_unless_ok(c, subgraph_impl(c, edges_out, scanned_out, ms_out));
}

int fora_hip_sparse_subgraph_fetch(fora_ctx *c, int64_t *sub_ptr, int32_t *sub_col, int64_t *sub_eid, uint64_t cap) {
    if (!c) return FORA_E_ARG;
    if (!c->sp.valid || !c->sp.compacted || !c->sb.valid) return fail(c, FORA_E_ARG, "sparse subgraph fetch: no subgraph is held");
    if (cap < c->sb.edges) return fail(c, FORA_E_ARG, "sparse subgraph fetch: cap is smaller than the held edges");
    HIPCHK(c, hipSetDevice(c->device));
    bool ptr_on_device = false, col_on_device = false, eid_on_device = false;
    if (sub_ptr) if (int rc = sparse_dest(c, sub_ptr, ptr_on_device)) return rc;
    if (sub_col) if (int rc = sparse_dest(c, sub_col, col_on_device)) return rc;
    if (sub_eid) if (int rc = sparse_dest(c, sub_eid, eid_on_device)) return rc;
    const uint64_t nc = c->sp.cols, edges = c->sb.edges;
    if (sub_ptr) {
        if (nc) HIPCHK(c, hipMemcpyAsync(sub_ptr, c->sb.d_ptr.get(), ((size_t)nc + 1) * 8, hipMemcpyDefault, c->stream));
        else if (ptr_on_device) HIPCHK(c, hipMemsetAsync(sub_ptr, 0, 8, c->stream)); // (nothing was launched: the one offset)
        else sub_ptr[0] = 0;
    }
    if (sub_col && edges) HIPCHK(c, hipMemcpyAsync(sub_col, c->sb.d_col.get(), (size_t)edges * 4, hipMemcpyDefault, c->stream));
    if (sub_eid && edges) HIPCHK(c, hipMemcpyAsync(sub_eid, c->sb.d_eid.get(), (size_t)edges * 8, hipMemcpyDefault, c->stream));
    return held_call_end(c, "sparse subgraph fetch", false);
}

// ---- SUBGRAPH PRODUCTS (the contract of include/fora_hip_gnn.h; kernels in fora_subgraph_prop.h, the split in fora_subgraph_prop_plan.h)
static_assert(SUB_SHORT_MAX == FORA_PROP_SEG, "a short row of SUBGRAPH PRODUCTS is one segment of the contract");
namespace {
// the transposition of the held subgraph: counts, the host's prefix sum, places, every column's keys sorted on the tiers of
// PROPAGATE, TRANSPOSED (a key is sub_key(row, place in the row), so a multi-edge's two entries keep the order of their places),
// then in_row and in_pos.  Complete or absent: built in locals, moved into SubBufs::prop after the last step.
int subt_build(fora_ctx *c) {
    SubBufs &b = c->sb;
    const uint64_t nc = c->sp.cols, edges = b.edges;
    DevBuf<int64_t> d_in_ptr, d_in_pos; DevBuf<int32_t> d_in_row;
    DevBuf<uint32_t> d_cnt; PinBuf<uint32_t> h_cnt; // counts per column, then the cursors of the place pass; their pinned landing area
    DevBuf<uint64_t> d_key; DevBuf<PropTRun> d_runs;
    std::vector<int64_t> h_in_ptr((size_t)nc + 1, 0);
    // ---- every buffer before the first launch
    const char *what = "the subgraph's transposition";
    if (int rc = prop_ensure(c, d_in_ptr, (size_t)nc + 1, what)) return rc;
    if (int rc = prop_ensure(c, d_in_row, (size_t)edges, what)) return rc;
    if (int rc = prop_ensure(c, d_in_pos, (size_t)edges, what)) return rc;
    if (int rc = prop_ensure(c, d_cnt, (size_t)nc, what)) return rc;
    if (int rc = prop_ensure(c, d_key, (size_t)edges, what)) return rc;
    if (int rc = prop_ensure(c, d_runs, (size_t)propt_max_runs(nc, edges), what)) return rc;
    if (h_cnt.alloc((size_t)std::max<uint64_t>(nc, 1)) != hipSuccess) { (void)hipGetLastError(); return fail(c, FORA_E_NOMEM, "no pinned memory for the subgraph's transposition"); }
    if (edges) {
        const uint32_t wgs = (uint32_t)std::min<uint64_t>(nc, 65535);
        const int64_t *sub_ptr = b.d_ptr.get();
        const int32_t *sub_col = b.d_col.get();
        EvSpan ev(c, EV_SUBP_T);
        HIPCHK(c, d_cnt.zero(c->stream, (size_t)nc));
        hipLaunchKernelGGL(k_subt_count, dim3(wgs), dim3(BLOCK), 0, c->stream, sub_ptr, (uint32_t)nc, sub_col, d_cnt.get());
        HIPCHK(c, hipMemcpyAsync(h_cnt.get(), d_cnt.get(), (size_t)nc * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); // (the counts are back)
        if (propt_scan(h_cnt.get(), (int64_t)nc, h_in_ptr.data()) != edges) return fail(c, FORA_E_HIP, "subgraph transpose: the counts do not add up to the held edges");
        const PropTTiers tiers = propt_tiers(h_in_ptr.data(), (int64_t)nc, c->opt_.propt_lds_cap);
        if (tiers.runs.size() > d_runs.size()) return fail(c, FORA_E_HIP, "subgraph transpose: more runs than the table holds");
        HIPCHK(c, hipMemcpyAsync(d_in_ptr.get(), h_in_ptr.data(), ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, c->stream));
        if (!tiers.runs.empty()) HIPCHK(c, hipMemcpyAsync(d_runs.get(), tiers.runs.data(), tiers.runs.size() * sizeof(PropTRun), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, d_cnt.zero(c->stream, (size_t)nc));
        hipLaunchKernelGGL(k_propt_place, dim3(wgs), dim3(BLOCK), 0, c->stream, sub_ptr, (uint32_t)nc, sub_col, (uint32_t)nc, (const int64_t *)d_in_ptr.get(), d_cnt.get(),
                           d_key.get(), edges);
        const PropTRun *r_short = d_runs.get(), *r_lds = r_short + tiers.n_short, *r_global = r_lds + tiers.n_lds;
        if (tiers.n_short) hipLaunchKernelGGL(k_propt_sort_short, dim3((tiers.n_short + BLOCK / 64 - 1) / (BLOCK / 64)), dim3(BLOCK), 0, c->stream, r_short, tiers.n_short, d_key.get());
        if (tiers.n_lds) hipLaunchKernelGGL(k_propt_sort_lds, dim3(tiers.n_lds), dim3(BLOCK), 0, c->stream, r_lds, d_key.get());
        if (tiers.n_global) {
            const uint32_t P = propt_pow2(tiers.max_global);
            const unsigned gx = (unsigned)std::min<uint32_t>(std::max<uint32_t>(1, P / 2 / BLOCK), 1024);
            for (uint32_t r0 = 0; r0 < tiers.n_global; r0 += 65535) { // (a grid's y extent)
                const dim3 grid(gx, std::min<uint32_t>(65535, tiers.n_global - r0));
                for (uint32_t k = 2; k <= P; k <<= 1) {
                    hipLaunchKernelGGL(k_propt_sort_step, grid, dim3(BLOCK), 0, c->stream, r_global + r0, d_key.get(), k, 0u);
                    for (uint32_t j = k >> 2; j; j >>= 1) hipLaunchKernelGGL(k_propt_sort_step, grid, dim3(BLOCK), 0, c->stream, r_global + r0, d_key.get(), k, j);
                }
            }
        }
        hipLaunchKernelGGL(k_subt_fill, dim3((unsigned)std::min<uint64_t>((edges + BLOCK - 1) / BLOCK, 8192)), dim3(BLOCK), 0, c->stream, (const uint64_t *)d_key.get(), edges,
                           sub_ptr, (uint32_t)nc, d_in_row.get(), d_in_pos.get());
        ev.end();
    } else HIPCHK(c, d_in_ptr.zero(c->stream, (size_t)nc + 1));
    if (int rc = held_call_end(c, "subgraph transpose")) return rc; // (idle: the tables go out of use)
    SubProp &p = b.prop;
    p.d_in_ptr = std::move(d_in_ptr); p.d_in_row = std::move(d_in_row); p.d_in_pos = std::move(d_in_pos);
    p.tr = SubProp::Side{};
    p.tr.h_ptr = std::move(h_in_ptr); p.tr.have_ptr = true;
    p.t_built = true; b.prop_used = true;
    return FORA_OK;
}
int subt_ensure(fora_ctx *c, bool &built_now) {
    built_now = false;
    if (c->sb.prop.t_built) return FORA_OK;
    if (int rc = subt_build(c)) return rc;
    built_now = true;
    return FORA_OK;
}
// the offsets of a side on the host: in_ptr came with the transposition, sub_ptr is copied once per held subgraph
int sub_side_ptr(fora_ctx *c, SubProp::Side &s) {
    if (s.have_ptr) return FORA_OK;
    const uint64_t nc = c->sp.cols;
    s.h_ptr.assign((size_t)nc + 1, 0);
    HIPCHK(c, hipMemcpy(s.h_ptr.data(), c->sb.d_ptr.get(), ((size_t)nc + 1) * 8, hipMemcpyDeviceToHost));
    s.have_ptr = true; c->sb.prop_used = true;
    return FORA_OK;
}
// the plan of a side's long rows under (cap, per), with its tables on the device: made when the key moves, kept otherwise
int sub_side_plan(fora_ctx *c, SubProp::Side &s, uint32_t cap, uint64_t per) {
    if (s.planned && s.cap == cap && s.per == per) return FORA_OK;
    s.planned = false;
    PropPlan plan = sub_long_plan(s.h_ptr.data(), (int)c->sp.cols, cap, per);
    if (int rc = prop_ensure(c, s.d_segs, plan.segs.size(), "the long rows' segment table")) return rc;
    if (int rc = prop_ensure(c, s.d_recs, plan.recs.size(), "the long rows' segment table")) return rc;
    if (!plan.segs.empty()) HIPCHK(c, hipMemcpy(s.d_segs.get(), plan.segs.data(), plan.segs.size() * sizeof(PropSeg), hipMemcpyHostToDevice));
    if (!plan.recs.empty()) HIPCHK(c, hipMemcpy(s.d_recs.get(), plan.recs.data(), plan.recs.size() * sizeof(PropRowRec), hipMemcpyHostToDevice));
    s.plan = std::move(plan); s.cap = cap; s.per = per; s.planned = true;
    return FORA_OK;
}
// one product over the held subgraph (forward: its rows; transposed: its columns).  nc > 0; the arguments have passed sub_prop_entry
int subgraph_prop_impl(fora_ctx *c, bool transposed, const void *x, int x_type, int d, int64_t ldx, int flags, const void *values, int val_type,
                       float *out32, double *out64, int64_t ldo, int64_t *info_out, double *ms_out) {
    SubBufs &b = c->sb;
    PropBufs &pb = c->pr;
    const uint64_t nc = c->sp.cols, edges = b.edges;
    const char *who = transposed ? "subgraph propagate_t" : "subgraph propagate";
    const uint32_t elt = elt_bytes(x_type);
    HeldIn feat = HeldIn::matrix(x, nc, ldx, (uint64_t)d, elt), vals = HeldIn::vector(values, edges, val_type == FORA_PROP_F64 ? 8 : 4);
    HeldOut<float> o32{out32, ldo, nc, (uint64_t)d};
    HeldOut<double> o64{out64, ldo, nc, (uint64_t)d};
    if (int rc = held_resolve(c, feat, vals, o32, o64)) return rc; // (before anything is built)
    c->tm.subp_t_ms = c->tm.subp_short_ms = c->tm.subp_long_ms = 0;
    bool built_now = false;
    if (transposed) if (int rc = subt_ensure(c, built_now)) return rc;
    SubProp &sp = b.prop;
    SubProp::Side &side = transposed ? sp.tr : sp.fwd;
    // ---- the split and, for the long rows, the plan: from the host copy of the offsets, kept with the subgraph
    const uint32_t cap = sub_short_cap(c->opt_.sub_short);
    if (int rc = sub_side_ptr(c, side)) return rc;
    if (!side.planned || side.cap != cap) { side.split = sub_split(side.h_ptr.data(), (int)nc, cap); side.planned = false; side.cap = cap; }
    const SubSplit split = side.split;
    const bool lng = split.long_rows != 0;
    uint64_t per = 1;
    if (lng) {
        size_t fr = 0, tot = 0;
        if (c->opt_.prop_segs <= 0) HIPCHK(c, hipMemGetInfo(&fr, &tot));
        per = prop_chunk_segs(c->opt_.prop_segs, split.long_segs, (uint64_t)fr, d);
    }
    // ---- every buffer of the call before the first launch: a call that finds no room has written nothing
    if (int rc = sub_side_plan(c, side, cap, per)) return rc;
    if (int rc = feat.stage(c, pb.d_feat, "the feature upload")) return rc;
    if (int rc = vals.stage(c, pb.d_vals, "the values upload")) return rc;
    if (lng) {
        if (int rc = prop_ensure(c, pb.d_part, (size_t)(per * (uint64_t)d), "the partial sums")) return rc;
        if (int rc = prop_ensure(c, pb.d_carry, 2 * (size_t)d, "the partial sums")) return rc;
        if (int rc = prop_ensure(c, pb.d_scarry, 2, "the partial sums")) return rc;
    }
    if (int rc = o32.reserve(c, pb.d_out32)) return rc;
    if (int rc = o64.reserve(c, pb.d_out64)) return rc;
    const PropGeom g = prop_geom((uint64_t)(uintptr_t)feat.ptr(), ldx, d, elt, prop_widths_bytes(elt), PROP_NWIDTHS);
    const int64_t *ptr = transposed ? sp.d_in_ptr.get() : b.d_ptr.get();
    const int32_t *ids = transposed ? sp.d_in_row.get() : b.d_col.get();
    const int64_t *pos = transposed && vals.ptr() ? sp.d_in_pos.get() : nullptr;
    const bool val64 = val_type == FORA_PROP_F64, mean = (flags & FORA_SUB_MEAN) != 0;
    if (split.short_rows) {
        EvSpan ev(c, EV_SUBP_SHORT);
        const uint64_t per_wg = (uint64_t)g.segs_per_wave * (BLOCK / 64);
        const dim3 grid((unsigned)((nc + per_wg - 1) / per_wg), g.tiles);
        const uint32_t wmode = vals.ptr() ? (val64 ? 2u : 1u) : 0u;
        with_vec(x_type, g.V, [&](auto E, auto V) {
            hipLaunchKernelGGL((k_sub_agg<E.value, V.value>), grid, dim3(BLOCK), 0, c->stream, ptr, (uint32_t)nc, cap, ids, pos, vals.ptr(), wmode, feat.ptr(), ldx, (uint32_t)d, g.G,
                               mean ? 1u : 0u, o32.ptr(), o32.ld(), o64.ptr(), o64.ld());
        });
    }
    if (lng) {
        EvSpan ev(c, EV_SUBP_LONG);
        const PropSide sd{side.h_ptr.data(), (int)nc, ids, nullptr, nullptr, false, vals.ptr(), val64, pos, vals.ptr() == nullptr};
        prop_launch_chunks(c, side.plan, side.d_segs.get(), side.d_recs.get(), sd, x_type, g, feat.ptr(), ldx, d, nullptr, o32.ptr(), o32.ld(), o64.ptr(), o64.ld(), false,
                           mean ? ptr : nullptr);
    }
    if (int rc = held_fetch(c, o32, o64)) return rc;
    if (int rc = held_call_end(c, who)) return rc;
    if (info_out) { info_out[0] = built_now ? 1 : 0; info_out[1] = (int64_t)split.long_rows; info_out[2] = lng ? (int64_t)side.plan.chunks.size() : 0; info_out[3] = feat.on_device(); }
    if (ms_out) { ms_out[0] = c->tm.subp_t_ms; ms_out[1] = c->tm.subp_short_ms; ms_out[2] = c->tm.subp_long_ms; }
    return FORA_OK;
}
int sub_prop_entry(fora_ctx *c, bool transposed, const void *x, int x_type, int d, int64_t ldx, int flags, const void *values, int val_type,
                   float *out32, double *out64, int64_t ldo, int64_t *info_out, double *ms_out) {
    if (!c) return FORA_E_ARG;
    const std::string who = transposed ? "subgraph propagate_t" : "subgraph propagate";
    if (!c->sp.valid || !c->sp.compacted || !c->sb.valid) return fail(c, FORA_E_ARG, who + ": no subgraph is held (fora_hip_sparse_subgraph first)");
    if (!elt_known(x_type)) return fail(c, FORA_E_ARG, who + ": unknown element type");
    if (flags & ~FORA_SUB_MEAN) return fail(c, FORA_E_ARG, who + ": unknown flag");
    if (d < 1 || d > 65536) return fail(c, FORA_E_ARG, who + ": d outside 1 .. 65536");
    if (ldx < d || ldo < d) return fail(c, FORA_E_ARG, who + ": a leading dimension smaller than d");
    if (!out32 && !out64) return fail(c, FORA_E_ARG, who + ": no output");
    if (c->sp.cols && !x) return fail(c, FORA_E_ARG, who + ": null operand");
    if (values) {
        if (flags & FORA_SUB_MEAN) return fail(c, FORA_E_ARG, who + ": FORA_SUB_MEAN with values");
        if (val_type != FORA_PROP_F32 && val_type != FORA_PROP_F64) return fail(c, FORA_E_ARG, who + ": val_type is neither f32 nor f64");
    }
    if (info_out) memset(info_out, 0, 4 * sizeof(int64_t));
    if (ms_out) memset(ms_out, 0, 3 * sizeof(double));
    if (!c->sp.cols) return FORA_OK; // (no output rows: nothing launched)
    HIPCHK(c, hipSetDevice(c->device));
    return drop_pairs_unless_ok(c, subgraph_prop_impl(c, transposed, x, x_type, d, ldx, flags, c->sb.edges ? values : nullptr, val_type, out32, out64, ldo, info_out, ms_out));
}
} // namespace

int fora_hip_subgraph_propagate(fora_ctx *c, const void *x, int x_type, int d, int64_t ldx, int flags, const void *values, int val_type,
                                float *out32, double *out64, int64_t ldo, int64_t *info_out, double *ms_out) {
    return sub_prop_entry(c, false, x, x_type, d, ldx, flags, values, val_type, out32, out64, ldo, info_out, ms_out);
}
int fora_hip_subgraph_propagate_t(fora_ctx *c, const void *g, int g_type, int d, int64_t ldg, int flags, const void *values, int val_type,
                                  float *out32, double *out64, int64_t ldo, int64_t *info_out, double *ms_out) {
    return sub_prop_entry(c, true, g, g_type, d, ldg, flags, values, val_type, out32, out64, ldo, info_out, ms_out);
}
int fora_hip_subgraph_transpose_fetch(fora_ctx *c, int64_t *in_ptr, int32_t *in_row, int64_t *in_pos, uint64_t cap) {
    if (!c) return FORA_E_ARG;
    if (!c->sp.valid || !c->sp.compacted || !c->sb.valid) return fail(c, FORA_E_ARG, "subgraph transpose fetch: no subgraph is held");
    if (cap < c->sb.edges) return fail(c, FORA_E_ARG, "subgraph transpose fetch: cap is smaller than the held edges");
    HIPCHK(c, hipSetDevice(c->device));
    bool ptr_on_device = false, row_on_device = false, pos_on_device = false;
    if (in_ptr) if (int rc = sparse_dest(c, in_ptr, ptr_on_device)) return rc;
    if (in_row) if (int rc = sparse_dest(c, in_row, row_on_device)) return rc;
    if (in_pos) if (int rc = sparse_dest(c, in_pos, pos_on_device)) return rc;
    const uint64_t nc = c->sp.cols, edges = c->sb.edges;
    if (!nc) { // (nothing is built or launched: the one offset)
        if (in_ptr) { if (ptr_on_device) HIPCHK(c, hipMemsetAsync(in_ptr, 0, 8, c->stream)); else in_ptr[0] = 0; }
        return held_call_end(c, "subgraph transpose fetch", false);
    }
    bool built_now = false;
    if (int rc = drop_pairs_unless_ok(c, subt_ensure(c, built_now))) return rc;
    const SubProp &p = c->sb.prop;
    if (in_ptr) HIPCHK(c, hipMemcpyAsync(in_ptr, p.d_in_ptr.get(), ((size_t)nc + 1) * 8, hipMemcpyDefault, c->stream));
    if (in_row && edges) HIPCHK(c, hipMemcpyAsync(in_row, p.d_in_row.get(), (size_t)edges * 4, hipMemcpyDefault, c->stream));
    if (in_pos && edges) HIPCHK(c, hipMemcpyAsync(in_pos, p.d_in_pos.get(), (size_t)edges * 8, hipMemcpyDefault, c->stream));
    return held_call_end(c, "subgraph transpose fetch", false);
}

// ---- ROW STORE (the contract of include/fora_hip.h; kernels in fora_store.h, the plan in fora_store_plan.h)
namespace {
// a plan on the device: out_ptr | src | win in the store's plan buffer
struct StorePlanDev { const int64_t *out_ptr = nullptr, *src = nullptr, *win = nullptr; };
int store_upload_plan(fora_ctx *c, const StorePlan &p, StorePlanDev &d) {
    RowStore &s = c->st;
    const size_t a = p.out_ptr.size(), b = p.src.size(), w = p.win.size();
    if (int rc = prop_ensure(c, s.d_plan, a + b + w, "the store's plan")) return rc;
    int64_t *at = s.d_plan.get();
    HIPCHK(c, hipMemcpyAsync(at, p.out_ptr.data(), a * 8, hipMemcpyHostToDevice, c->stream));
    if (b) HIPCHK(c, hipMemcpyAsync(at + a, p.src.data(), b * 8, hipMemcpyHostToDevice, c->stream));
    if (w) HIPCHK(c, hipMemcpyAsync(at + a + b, p.win.data(), w * 8, hipMemcpyHostToDevice, c->stream));
    d.out_ptr = at; d.src = at + a; d.win = at + a + b;
    return FORA_OK;
}
inline unsigned store_grid(uint64_t spans) { return (unsigned)std::min<uint64_t>(spans, 1u << 20); } // (the kernels stride over the spans)

// where a put / load writes: behind the store's entries when an append fits there, otherwise into new arrays that start with a
// copy of the rows that stay -- moved into the store by store_commit, freed on every other way out
struct StoreDest {
    DevBuf<int32_t> ids; DevBuf<uint64_t> fix; bool fresh = false;
    int32_t *p_ids = nullptr; uint64_t *p_fix = nullptr; uint64_t base = 0; // the arrays, and the first entry the call writes
};
int store_dest(fora_ctx *c, bool append, uint64_t add, StoreDest &d) {
    RowStore &s = c->st;
    d.base = append ? s.entries : 0;
    const uint64_t total = d.base + add;
    if (append && total <= std::min<uint64_t>(s.d_ids.size(), s.d_fix.size())) { d.p_ids = s.d_ids.get(); d.p_fix = s.d_fix.get(); return FORA_OK; }
    d.fresh = true;
    for (uint64_t cap = d.base ? std::max(total, d.base + d.base / 2) : total;; cap = total) { // (an append grows by half at least; a guess that does not fit is no reason to fail)
        if (d.ids.alloc((size_t)std::max<uint64_t>(cap, 1)) == hipSuccess && d.fix.alloc((size_t)std::max<uint64_t>(cap, 1)) == hipSuccess) break;
        (void)hipGetLastError(); d.ids.reset(); d.fix.reset();
        if (cap == total) return fail(c, FORA_E_NOMEM, "no device memory for the row store");
    }
    d.p_ids = d.ids.get(); d.p_fix = d.fix.get();
    if (d.base) {
        HIPCHK(c, hipMemcpyAsync(d.p_ids, s.d_ids.get(), d.base * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d.p_fix, s.d_fix.get(), d.base * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    return FORA_OK;
}
// the last step of a put / load, behind an idle stream: nothing fails from here on
void store_commit(fora_ctx *c, StoreDest &d, bool append, const int64_t *row_ptr, int64_t nrows, uint64_t max_row) {
    RowStore &s = c->st;
    if (!append || s.h_row_ptr.empty()) { s.h_row_ptr.assign(1, 0); s.entries = 0; s.max_row = 0; }
    if (d.fresh) { s.d_ids = std::move(d.ids); s.d_fix = std::move(d.fix); }
    for (int64_t i = 1; i <= nrows; i++) s.h_row_ptr.push_back((int64_t)d.base + row_ptr[i]);
    s.entries = d.base + (uint64_t)row_ptr[nrows];
    s.max_row = std::max(s.max_row, max_row);
}

// what put and load share: nrows rows of (row_ptr, ids, fix) become the store, or its rows R ..; ids / fix on the device or the
// host; check: every entry is validated on the device before anything moves (load; the rows of a held result are valid)
int store_add(fora_ctx *c, const char *who, const int64_t *row_ptr, int64_t nrows, const int32_t *ids, bool ids_dev, const uint64_t *fix, bool fix_dev, bool check,
              bool append, fora_store_stats *st) {
    RowStore &s = c->st;
    const uint64_t entries = (uint64_t)row_ptr[nrows];
    uint64_t max_row = 0;
    for (int64_t i = 0; i < nrows; i++) max_row = std::max(max_row, (uint64_t)(row_ptr[i + 1] - row_ptr[i]));
    s.h_row_ptr.reserve((append ? s.h_row_ptr.size() : 0) + (size_t)nrows + 1);
    StorePlan plan; StorePlanDev pd;
    unsigned long long bad = ~0ull;
    // ---- every buffer before the first launch
    StoreDest d;
    if (check && entries) {
        plan = store_take_plan(row_ptr, nullptr, nrows, store_span(c->opt_.take_span));
        if (int rc = prop_ensure(c, s.d_bad, 1, "the store's check")) return rc;
        if (int rc = store_upload_plan(c, plan, pd)) return rc;
        HIPCHK(c, hipMemsetAsync(s.d_bad.get(), 0xFF, sizeof(bad), c->stream));
    }
    if (int rc = store_dest(c, append, entries, d)) return rc;
    c->tm.store_ms = 0;
    if (entries) {
        EvSpan ev(c, EV_STORE);
        HIPCHK(c, hipMemcpyAsync(d.p_ids + d.base, ids, entries * 4, ids_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d.p_fix + d.base, fix, entries * 8, fix_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        if (check) hipLaunchKernelGGL(k_store_check, dim3(store_grid(plan.spans)), dim3(BLOCK), 0, c->stream, pd.out_ptr, pd.win, plan.spans, entries, plan.span,
                                      (const int32_t *)(d.p_ids + d.base), (uint32_t)c->g.n, s.d_bad.get());
        ev.end();
        if (check) HIPCHK(c, hipMemcpyAsync(&bad, s.d_bad.get(), sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    }
    if (int rc = held_call_end(c, who)) return rc; // (idle: the check has finished, the plan and the caller's arrays go out of use)
    if (bad != ~0ull) {
        const int64_t row = (int64_t)(std::upper_bound(row_ptr, row_ptr + nrows + 1, (int64_t)bad) - row_ptr) - 1;
        return fail(c, FORA_E_ARG, std::string(who) + ": entry " + std::to_string(bad) + " (row " + std::to_string(row) + ", place " + std::to_string((int64_t)bad - row_ptr[row]) +
                                       "): an id outside [0, n), or not above the id before it in its row");
    }
    store_commit(c, d, append, row_ptr, nrows, max_row);
    if (st) {
        st->rows = (uint64_t)nrows; st->entries = entries; st->max_row = max_row;
        st->store_rows = (uint64_t)s.rows(); st->store_entries = s.entries;
        st->ids_on_device = ids_dev ? 1 : 0; st->fix_on_device = fix_dev ? 1 : 0;
        st->store_ms = c->tm.store_ms;
    }
    return FORA_OK;
}

int store_take_impl(fora_ctx *c, const int64_t *rows, int nb, int64_t *row_ptr_out, fora_store_stats *st) {
    RowStore &s = c->st;
    const StorePlan plan = store_take_plan(s.h_row_ptr.data(), rows, nb, store_span(c->opt_.take_span));
    // ---- every buffer before the launch: no room leaves nothing held and the store as it was
    const size_t room = (size_t)std::max<uint64_t>(plan.entries, 1);
    if (c->sp.d_ids.ensure(room) != hipSuccess || c->sp.d_fix.ensure(room) != hipSuccess) {
        (void)hipGetLastError(); c->sp.d_ids.reset(); c->sp.d_fix.reset();
        return fail(c, FORA_E_NOMEM, "store take: no device memory for the result");
    }
    StorePlanDev pd;
    c->tm.store_ms = 0;
    if (plan.entries) {
        if (int rc = store_upload_plan(c, plan, pd)) return rc;
        EvSpan ev(c, EV_STORE);
        hipLaunchKernelGGL(k_store_take, dim3(store_grid(plan.spans)), dim3(BLOCK), 0, c->stream, pd.out_ptr, pd.src, pd.win, plan.spans, plan.entries, plan.span,
                           (const int32_t *)s.d_ids.get(), (const uint64_t *)s.d_fix.get(), s.entries, c->sp.d_ids.get(), c->sp.d_fix.get(),
                           (uint64_t)std::min(c->sp.d_ids.size(), c->sp.d_fix.size()));
    }
    RowLayout lay; // every row placed by the plan, none dangling: the end of a call that made a held result
    lay.begin(nullptr, nb);
    lay.row_ptr = plan.out_ptr; lay.cur = plan.entries; lay.max_row = plan.max_row;
    if (int rc = finish_rows(c, lay, c->sp, "store take", row_ptr_out, [](uint32_t, const int64_t *, const int32_t *) {})) return rc;
    if (st) {
        st->rows = (uint64_t)nb; st->entries = plan.entries; st->max_row = plan.max_row;
        st->store_rows = (uint64_t)s.rows(); st->store_entries = s.entries;
        st->store_ms = c->tm.store_ms;
    }
    return FORA_OK;
}
} // namespace

int fora_hip_store_put(fora_ctx *c, const int64_t *row_ptr, int nq, int append, fora_store_stats *st) {
    if (int rc = held_call_begin(c, "store put", row_ptr, nq)) return rc;
    if (c->sp.compacted) return fail(c, FORA_E_ARG, "store put: the held result is compacted (the store holds node ids)");
    if (st) memset(st, 0, sizeof(*st));
    HIPCHK(c, hipSetDevice(c->device));
    return drop_pairs_unless_ok(c, store_add(c, "store put", row_ptr, nq, c->sp.d_ids.get(), true, c->sp.d_fix.get(), true, false, append != 0, st));
}

int fora_hip_store_load(fora_ctx *c, const int64_t *row_ptr, int64_t nrows, const int32_t *ids, const uint64_t *fix, int append, fora_store_stats *st) {
    if (!c) return FORA_E_ARG;
    if (!c->g.n) return fail(c, FORA_E_ARG, "store load: set_graph first");
    if (nrows < 0 || !row_ptr) return fail(c, FORA_E_ARG, "store load: negative nrows or null row_ptr");
    if (!store_row_ptr_ok(row_ptr, nrows)) return fail(c, FORA_E_ARG, "store load: row_ptr does not start at 0 or decreases");
    if (row_ptr[nrows] && (!ids || !fix)) return fail(c, FORA_E_ARG, "store load: null ids or fix");
    if (st) memset(st, 0, sizeof(*st));
    HIPCHK(c, hipSetDevice(c->device));
    bool ids_dev = false, fix_dev = false;
    if (ids) if (int rc = sparse_dest(c, ids, ids_dev)) return rc;
    if (fix) if (int rc = sparse_dest(c, fix, fix_dev)) return rc;
    return drop_pairs_unless_ok(c, store_add(c, "store load", row_ptr, nrows, ids, ids_dev, fix, fix_dev, true, append != 0, st));
}

int fora_hip_store_take(fora_ctx *c, const int64_t *rows, int nb, int64_t *row_ptr_out, fora_store_stats *st) {
    if (!c) return FORA_E_ARG;
    uint64_t thr;
    if (int rc = held_rows_begin(c, c->sp, row_ptr_out, 0.0, thr)) return rc; // (the held result has ended; a null row_ptr_out is refused there)
    if (st) memset(st, 0, sizeof(*st));
    if (nb < 0 || (nb > 0 && !rows)) return fail(c, FORA_E_ARG, "store take: negative nb or null rows");
    const int64_t bad = store_bad_index(rows, nb, c->st.rows());
    if (bad >= 0) return fail(c, FORA_E_ARG, "store take: rows[" + std::to_string(bad) + "] = " + std::to_string(rows[bad]) + " is outside the store's " + std::to_string(c->st.rows()) + " rows");
    HIPCHK(c, hipSetDevice(c->device));
    return drop_pairs_unless_ok(c, store_take_impl(c, rows, nb, row_ptr_out, st));
}

int fora_hip_store_info(fora_ctx *c, int64_t *rows, uint64_t *entries, uint64_t *max_row) {
    if (!c) return FORA_E_ARG;
    if (rows) *rows = c->st.rows();
    if (entries) *entries = c->st.entries;
    if (max_row) *max_row = c->st.max_row;
    return FORA_OK;
}

int fora_hip_store_clear(fora_ctx *c) {
    if (!c) return FORA_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_store(c);
    return FORA_OK;
}

int fora_hip_push_batch(fora_ctx *c, const int32_t *sources, int nq, uint64_t *reserve_fix_out,
                        uint64_t *residue_fix_out, fora_query_stats *stats) {
    return with_bucket_retry(c, [&] { return query_common(c, sources, nq, 0, RUN_PUSH_ONLY, nullptr, reserve_fix_out, residue_fix_out, stats); });
}

int fora_hip_walk_counts(fora_ctx *c, const double *residue, double rsum, uint64_t *num_s_rw, uint64_t *n_rw) {
    if (!c || !c->g.n || !c->par.have || !residue || !num_s_rw) return fail(c, FORA_E_ARG, "bad call");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> d_r; DevBuf<uint64_t> d_num, d_n;
    const size_t n = (size_t)c->g.n;
    HIPCHK(c, d_r.alloc(n));
    HIPCHK(c, d_num.alloc(n));
    HIPCHK(c, d_n.alloc(1));
    HIPCHK(c, hipMemcpy(d_r.get(), residue, n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_walk_counts_f64, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream,
                       c->g.n, (const double *)d_r.get(), rsum, c->par.omega, c->par.alpha, c->par.opt, d_num.get(), d_n.get());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(num_s_rw, d_num.get(), n * 8, hipMemcpyDeviceToHost));
    uint64_t N = 0;
    HIPCHK(c, hipMemcpy(&N, d_n.get(), 8, hipMemcpyDeviceToHost));
    if (n_rw) *n_rw = N;
    return FORA_OK;
}

int fora_hip_walks(fora_ctx *c, uint32_t stream_id, uint32_t round, int no_zero_hop, const int32_t *starts,
                   const uint64_t *js, int64_t count, int32_t *dests) {
    if (!c || !c->g.n || !c->par.have || count < 0) return fail(c, FORA_E_ARG, "bad call");
    if (count == 0) return FORA_OK;
    for (int64_t i = 0; i < count; i++)
        if (starts[i] < 0 || starts[i] >= c->g.n) return fail(c, FORA_E_ARG, "walk start out of range");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<int32_t> d_s, d_d; DevBuf<uint64_t> d_j;
    HIPCHK(c, d_s.alloc((size_t)count));
    HIPCHK(c, d_d.alloc((size_t)count));
    HIPCHK(c, d_j.alloc((size_t)count));
    HIPCHK(c, hipMemcpy(d_s.get(), starts, (size_t)count * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_j.get(), js, (size_t)count * 8, hipMemcpyHostToDevice));
    Dev d{};
    d.n = c->g.n; d.rowinfo = c->g.d_rowinfo.get(); d.row_ptr = c->g.d_row_ptr.get(); d.col = c->g.d_col.get();
    d.alpha32 = (uint32_t)(c->par.alpha * 4294967296.0);
    d.seed_lo = (uint32_t)c->par.seed; d.seed_hi = (uint32_t)(c->par.seed >> 32);
    hipLaunchKernelGGL(k_walks_raw, dim3((unsigned)((count + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, d,
                       stream_id, round, no_zero_hop, (const int32_t *)d_s.get(), (const uint64_t *)d_j.get(), count, d_d.get());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dests, d_d.get(), (size_t)count * 4, hipMemcpyDeviceToHost));
    return FORA_OK;
}

// top-k driver: fora_query_topk_new (query.h:972-1045) for a batch of slots (frame: topk_batch_start / topk_round /
// topk_batch_end).
static int topk_batch_impl(fora_ctx *c, const int32_t *sources, int nq, int k, double epsilon, double rmax_scale,
                           int with_idx, int32_t *ids, double *scores, int32_t *rounds);
int fora_hip_topk_batch(fora_ctx *c, const int32_t *sources, int nq, int k, double epsilon, double rmax_scale,
                        int with_idx, int32_t *ids, double *scores, int32_t *rounds) {
    return with_bucket_retry(c, [&] { return topk_batch_impl(c, sources, nq, k, epsilon, rmax_scale, with_idx, ids, scores, rounds); });
}
// checks of both drivers (but the range of the sources)
static int check_topk_args(fora_ctx *c, const int32_t *sources, int nq, int k, double epsilon, double rmax_scale, int with_idx,
                           const int32_t *ids, const double *scores) {
    if (int rc = check_batch_args(c, sources, nq)) return rc;
    if (nq && (!ids || !scores)) return fail(c, FORA_E_ARG, "ids / scores missing");
    if (k < 2 || k >= c->g.n - 1) return fail(c, FORA_E_ARG, "k out of range (query.h:1317-1318)");
    if (int rc = check_k(c, k)) return rc;
    if (!(epsilon > 0) || !(rmax_scale >= 0)) return fail(c, FORA_E_ARG, "bad epsilon / rmax_scale");
    if (with_idx && !c->ix.have) return fail(c, FORA_E_ARG, "with_idx without an index");
    return FORA_OK;
}
static int topk_batch_impl(fora_ctx *c, const int32_t *sources, int nq, int k, double epsilon, double rmax_scale,
                           int with_idx, int32_t *ids, double *scores, int32_t *rounds) {
    if (k == 0) k = 500; // query.h:975
    if (int rc = check_topk_args(c, sources, nq, k, epsilon, rmax_scale, with_idx, ids, scores)) return rc;
    if (int rc = check_id_range(c, sources, nq)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const double min_delta = 1.0 / c->g.n;           // query.h:974
    const double init_delta = 1.0 / k / 10;        // query.h:976
    const double pfail = 1.0 / c->g.n / c->g.n;        // query.h:977
    const long long m = c->g.m_attr;
    if (!(init_delta >= min_delta)) { // k > n/10: the reference's round loop (query.h:1001) never runs, topk_ppr sees an empty ppr
        for (size_t i = 0; i < (size_t)nq * k; i++) { ids[i] = 0; scores[i] = 0.0; }
        if (rounds) for (int i = 0; i < nq; i++) rounds[i] = 0;
        return FORA_OK;
    }
    // omega of the last possible round bounds the walk work list
    const double omega_max = (2 + epsilon) * log(2 / pfail) / min_delta / epsilon / epsilon;
    c->retry.div = want_wide(c) && c->opt_.bkcap <= 0 ? (uint32_t)std::max<int64_t>(1, c->opt_.topk_bk_div) : 1u;
    int rc = ensure_workspace(c, nq, omega_max);
    if (rc) return rc;
    if ((rc = ensure_topk_slabs(c, k))) return rc;
    const uint32_t chunks = slab_grid_x(c, std::min(nq, c->ws.B));
    TopkBatch tb{EvSpan(c)};
    std::vector<unsigned long long> above;
    const int per = even_batch(nq, c->ws.B);
    for (int b0 = 0; b0 < nq; b0 += per) {
        const int nb = std::min(per, nq - b0);
        if ((rc = topk_batch_start(c, tb, sources + b0, nb, with_idx != 0, chunks))) return rc;
        std::vector<double> sel_thr((size_t)nb, 0.0); // slots that stop with k entries >= T: the top k are among those
        double delta = init_delta;
        int round = 0;
        while (delta >= min_delta) { // query.h:1001
            if (std::find(tb.active.begin(), tb.active.end(), 1) == tb.active.end()) break;
            round++;
            // fora_topk_setting, algo.h:466-474
            double rmax = epsilon * sqrt(delta / 3 / m / log(2 / pfail));
            rmax *= sqrt(1.0 * m * rmax) * rmax_scale * 3;
            const double omega = (2 + epsilon) * log(2 / pfail) / delta / epsilon / epsilon;
            Dev dw{};
            if ((rc = topk_round<ALLOC_TOPK>(c, tb, nb, with_idx != 0, round, rmax, omega, chunks, nullptr, with_idx ? 1 : 0, dw))) return rc;
            const double T = (1 + epsilon) * delta; // query.h:1030
            EvSpan ev(c, EV_OTHER);
            hipLaunchKernelGGL(k_count_above, dim3(std::min<uint32_t>(chunks, 256), nb), dim3(BLOCK), 0, c->stream, dw,
                               (const uint8_t *)c->ws.d_active.get(), T, c->ws.d_above.get());
            ev.end();
            above.assign((size_t)nb, 0);
            HIPCHK(c, hipMemcpyAsync(above.data(), c->ws.d_above.get(), (size_t)nb * 8, hipMemcpyDeviceToHost, c->stream));
            if ((rc = check_dev_err(c))) return rc;
            for (int i = 0; i < nb; i++)
                if (tb.active[i] && (above[i] >= (unsigned long long)k || delta <= min_delta)) {
                    tb.active[i] = 0;
                    if (above[i] >= (unsigned long long)k) sel_thr[i] = T;
                }
            if (delta <= min_delta) break;
            delta = std::max(min_delta, delta / 4.0); // query.h:1041
        }
        if ((rc = topk_batch_end(c, tb, nb, k, sel_thr.data(), "topk", b0, ids, scores, rounds))) return rc;
    }
    return FORA_OK;
}

// top-k with bounds: fora_query_topk_with_bound (query.h:909-969) for a batch of slots, in the frame of the --opt driver
// (delta halves per round).  zero_ppr_upper_bound (query.h:935, :748) only ever feeds itself in the reference and is not kept.
static int topk_bound_batch_impl(fora_ctx *c, const int32_t *sources, int nq, int k, double epsilon, double rmax_scale,
                                 double ppr_decay_alpha, int with_idx, int32_t *ids, double *scores, int32_t *rounds);
int fora_hip_topk_bound_batch(fora_ctx *c, const int32_t *sources, int nq, int k, double epsilon, double rmax_scale,
                              double ppr_decay_alpha, int with_idx, int32_t *ids, double *scores, int32_t *rounds) {
    return with_bucket_retry(c, [&] {
        return topk_bound_batch_impl(c, sources, nq, k, epsilon, rmax_scale, ppr_decay_alpha, with_idx, ids, scores, rounds);
    });
}
static int topk_bound_batch_impl(fora_ctx *c, const int32_t *sources, int nq, int k, double epsilon, double rmax_scale,
                                 double ppr_decay_alpha, int with_idx, int32_t *ids, double *scores, int32_t *rounds) {
    if (int rc = check_topk_args(c, sources, nq, k, epsilon, rmax_scale, with_idx, ids, scores)) return rc;
    if (!(ppr_decay_alpha > 0 && ppr_decay_alpha < 1)) return fail(c, FORA_E_ARG, "bad ppr_decay_alpha");
    if (int rc = check_id_range(c, sources, nq)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const double min_delta = 1.0 / c->g.n;                                                                    // query.h:911
    const double init_delta = 1.0 / 4;                                                                      // :912
    const double threshold = (1.0 - ppr_decay_alpha) / pow(500, ppr_decay_alpha) / pow(c->g.n, 1 - ppr_decay_alpha); // :913
    const double pfail = 1.0 / c->g.n / c->g.n / log(c->g.n);                                                     // :915
    const double L = log(2 / pfail);
    const long long m = c->g.m_attr;
    const double omega_max = (2 + epsilon) * L / min_delta / epsilon / epsilon;
    c->retry.div = 1;
    int rc = ensure_workspace(c, nq, omega_max);
    if (rc) return rc;
    if ((rc = ensure_topk_slabs(c, k))) return rc;
    Workspace &w = c->ws;
    const uint64_t slab = (uint64_t)w.B * (uint64_t)c->g.n;
    HIPCHK(c, w.d_upper.ensure(slab));
    HIPCHK(c, w.d_lower.ensure(slab));
    if (!w.d_filter) { HIPCHK(c, w.d_filter.alloc(slab)); HIPCHK(c, w.d_filter.zero(c->stream)); } // the marks start from zero, once
    HIPCHK(c, w.d_fail.ensure((size_t)w.B));
    HIPCHK(c, w.d_round_walks.ensure((size_t)w.B));
    if ((rc = grow_pair(c, k, w.d_lb_ids, w.d_lb_sc))) return rc;
    const uint32_t chunks = slab_grid_x(c, std::min(nq, c->ws.B));
    TopkBatch tb{EvSpan(c)};
    std::vector<unsigned long long> above;
    std::vector<uint32_t> failv;
    const int per = even_batch(nq, c->ws.B);
    for (int b0 = 0; b0 < nq; b0 += per) {
        const int nb = std::min(per, nq - b0);
        if ((rc = topk_batch_start(c, tb, sources + b0, nb, with_idx != 0, chunks))) return rc;
        hipLaunchKernelGGL(k_bounds_reset, dim3(chunks, nb), dim3(BLOCK), 0, c->stream, c->g.n, c->ws.d_upper.get(), c->ws.d_lower.get()); // :941-942
        double delta = init_delta;
        int round = 0;
        while (delta >= min_delta) { // query.h:944
            if (std::find(tb.active.begin(), tb.active.end(), 1) == tb.active.end()) break;
            round++;
            double rmax = epsilon * sqrt(delta / 3 / m / L); // fora_setting with the round's delta, algo.h:455-463
            rmax *= rmax_scale;
            const double omega = (2 + epsilon) * L / delta / epsilon / epsilon;
            HIPCHK(c, c->ws.d_fail.zero(c->stream, (size_t)nb));
            HIPCHK(c, c->ws.d_round_walks.zero(c->stream, (size_t)nb));
            Dev dw{};
            if ((rc = topk_round<ALLOC_BOUND>(c, tb, nb, with_idx != 0, round, rmax, omega, chunks, c->ws.d_round_walks.get(), 0, dw))) return rc;
            EvSpan ev(c, EV_OTHER);
            if (delta < threshold) // query.h:745-746
                hipLaunchKernelGGL(k_bounds_update, dim3(chunks, nb), dim3(BLOCK), 0, c->stream, dw, (const uint64_t *)c->ws.d_ppr.get(),
                                   (const uint8_t *)c->ws.d_active.get(), (const unsigned long long *)c->ws.d_round_walks.get(), L,
                                   1.0 / c->g.n, sqrt(1.0 / c->g.n), c->ws.d_upper.get(), c->ws.d_lower.get());
            // if_stop, algo.h:1096-1166
            hipLaunchKernelGGL(k_count_above, dim3(std::min<uint32_t>(chunks, 256), nb), dim3(BLOCK), 0, c->stream, dw,
                               (const uint8_t *)c->ws.d_active.get(), 2.0 * delta, c->ws.d_above.get());
            const bool bounds_on = !(delta >= threshold);
            if (bounds_on) {
                Dev dl = dw;
                dl.ppr = (uint64_t *)c->ws.d_lower.get(); // non-negative f64: bit patterns order like the values
                if ((rc = launch_select(c, dl, nb, k, c->ws.d_lb_ids.get(), c->ws.d_lb_sc.get(), 1))) return rc;
                hipLaunchKernelGGL(k_bound_ratio, dim3(nb), dim3(SEL_THREADS), 0, c->stream, dw, k, (const int32_t *)c->ws.d_lb_ids.get(),
                                   (const double *)c->ws.d_lb_sc.get(), (const uint8_t *)c->ws.d_active.get(), (const double *)c->ws.d_upper.get(),
                                   1.0 + epsilon, c->ws.d_filter.get(), c->ws.d_fail.get());
                hipLaunchKernelGGL(k_bound_scan, dim3(chunks, nb), dim3(BLOCK), 0, c->stream, dw, k, (const double *)c->ws.d_lb_sc.get(),
                                   (const uint8_t *)c->ws.d_active.get(), (const double *)c->ws.d_upper.get(), (const double *)c->ws.d_lower.get(), delta,
                                   1.0 + epsilon, (1 + epsilon) / (1 - epsilon), c->ws.d_filter.get(), c->ws.d_fail.get());
            }
            ev.end();
            above.assign((size_t)nb, 0);
            failv.assign((size_t)nb, 0);
            HIPCHK(c, hipMemcpyAsync(above.data(), c->ws.d_above.get(), (size_t)nb * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(failv.data(), c->ws.d_fail.get(), (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
            if ((rc = check_dev_err(c))) return rc;
            for (int i = 0; i < nb; i++) {
                if (!tb.active[i]) continue;
                const bool stop = above[i] >= (unsigned long long)k || (bounds_on && failv[i] == 0);
                if (stop || delta <= min_delta) tb.active[i] = 0; // query.h:962-964
            }
            if (delta <= min_delta) break;
            delta = std::max(min_delta, delta / 2.0); // query.h:966
        }
        if ((rc = topk_batch_end(c, tb, nb, k, nullptr, "topk (bounds)", b0, ids, scores, rounds))) return rc;
    }
    return FORA_OK;
}

// gen_exact_topk's kernel (query.h:1192-1238): the push with threshold = one unit per out-edge and a fixed
// number of levels; what it reserves is the exact PPR up to (1-alpha)^max_iter.
static int power_iteration_batch_impl(fora_ctx *c, const int32_t *sources, int nq, int max_iter, double *ppr_out,
                                      uint64_t *ppr_fix_out, int k, int32_t *ids, double *scores);
int fora_hip_power_iteration_batch(fora_ctx *c, const int32_t *sources, int nq, int max_iter, double *ppr_out,
                                   uint64_t *ppr_fix_out, int k, int32_t *ids, double *scores) {
    return with_bucket_retry(c, [&] { return power_iteration_batch_impl(c, sources, nq, max_iter, ppr_out, ppr_fix_out, k, ids, scores); });
}
static int power_iteration_batch_impl(fora_ctx *c, const int32_t *sources, int nq, int max_iter, double *ppr_out,
                                      uint64_t *ppr_fix_out, int k, int32_t *ids, double *scores) {
    if (int rc = check_batch_args(c, sources, nq)) return rc;
    if (max_iter < 1 || max_iter >= MAX_LEVELS) return fail(c, FORA_E_ARG, "max_iter out of range");
    const bool want_topk = ids || scores;
    if (want_topk && (!ids || !scores)) return fail(c, FORA_E_ARG, "ids and scores go together");
    if (want_topk) if (int rc = check_k(c, k)) return rc;
    if (int rc = check_id_range(c, sources, nq)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_query_workspace(c, nq, want_topk ? k : 0);
    if (rc) return rc;
    const int per = even_batch(nq, c->ws.B);
    for (int b0 = 0; b0 < nq; b0 += per) {
        const int nb = std::min(per, nq - b0);
        EvSpan batch(c, EV_BATCH);
        if ((rc = reset_batch_state(c, nb, sources + b0))) return rc;
        Dev d = make_dev(c, nb, false, 0.0, c->par.omega); // rmax 0 -> threshold of one unit per out-edge
        hipLaunchKernelGGL(k_init_batch, dim3((nb + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, d, 2);
        if ((rc = run_push_levels(c, d, nullptr, max_iter))) return rc;
        if (want_topk) {
            EvSpan ev(c, EV_OTHER);
            if ((rc = launch_select(c, d, nb, k, c->ws.d_topk_ids.get(), c->ws.d_topk_sc.get(), 0))) return rc;
        }
        if ((rc = close_batch(c, &batch, "power iteration"))) return rc;
        if (want_topk && (rc = copy_topk_out(c, nb, k, ids, scores, (uint64_t)b0))) return rc;
        if ((rc = copy_slab_out(c, c->ws.d_ppr.get(), 0, (uint64_t)b0, (uint64_t)nb, ppr_fix_out, ppr_out, 62))) return rc;
    }
    return FORA_OK;
}

// ---- baselines of the reference's experiments: --algo montecarlo (query.h:1482-1493) and --algo fwdpush (:1495-1511)
static int check_baseline_args(fora_ctx *c, const int32_t *sources, int nq, double epsilon, int k) {
    if (int rc = check_batch_args(c, sources, nq)) return rc;
    if (!(epsilon > 0)) return fail(c, FORA_E_ARG, "epsilon must be > 0");
    if (k != 0) if (int rc = check_k(c, k)) return rc; // (0: no top-k)
    return check_id_range(c, sources, nq);
}

// FwdPush: the push of the FORA path at fwdpush_setting's rmax (algo.h:485-496), ppr = the reserve
// (compute_ppr_with_reserve, query.h:243-253).  The ctx's own rmax (and --balanced) are put back when the call returns.
struct PushRmaxScope {
    fora_ctx *c;
    double rmax;
    bool balanced;
    PushRmaxScope(fora_ctx *ctx, double r) : c(ctx), rmax(ctx->par.rmax), balanced(ctx->bal.on) { c->par.rmax = r; c->bal.on = false; }
    ~PushRmaxScope() { c->par.rmax = rmax; c->bal.on = balanced; }
};
static int fwdpush_batch_impl(fora_ctx *c, const int32_t *sources, int nq, double epsilon, double rmax_scale, double *ppr_out,
                              uint64_t *reserve_fix_out, uint64_t *residue_fix_out, int k, int32_t *ids, double *scores,
                              fora_query_stats *stats) {
    if (int rc = check_baseline_args(c, sources, nq, epsilon, k)) return rc;
    if (c->g.m_attr <= 0) return fail(c, FORA_E_ARG, "m of the graph must be > 0");
    const double delta = 1.0 / c->g.n;
    const double rmax = rmax_scale * delta * epsilon * c->g.n / c->g.m_attr; // config.rmax_scale*config.delta*config.epsilon*n/m
    if (!(rmax > 0) || !std::isfinite(rmax)) return fail(c, FORA_E_ARG, "rmax_scale must be > 0");
    PushRmaxScope scope(c, rmax);
    return query_common(c, sources, nq, 0, RUN_PUSH_ONLY, ppr_out, reserve_fix_out, residue_fix_out, stats, k, ids, scores);
}

int fora_hip_fwdpush_batch(fora_ctx *c, const int32_t *sources, int nq, double epsilon, double rmax_scale, double *ppr_out,
                           uint64_t *reserve_fix_out, uint64_t *residue_fix_out, int k, int32_t *ids, double *scores,
                           fora_query_stats *stats) {
    return with_bucket_retry(c, [&] {
        return fwdpush_batch_impl(c, sources, nq, epsilon, rmax_scale, ppr_out, reserve_fix_out, residue_fix_out, k, ids, scores, stats);
    });
}

// ---- backward push (reverse_local_update_linear, algo.h:703-751) and --algo bippr (bippr_query, query.h:71-124; bippr_query_topk
// :126-193).  The pushes run in two passes over the call's targets: a count pass (entries per target, counters, the targets
// that overflow the LDS tier) and, chunk by chunk, a write pass that runs the same pushes again and writes their entries
// target-major.  Chunks follow from the counts, so no chunk boundary depends on anything but the entry budget.
static int ensure_reverse_csr(fora_ctx *c) {
    if (c->g.rev.d_rin_ptr) return FORA_OK;
    const uint64_t n = (uint64_t)c->g.n, nnz = (uint64_t)c->g.nnz;
    DevBuf<uint32_t> indeg; DevBuf<unsigned long long> cursor;
    HIPCHK(c, indeg.alloc(n));
    HIPCHK(c, indeg.zero(c->stream));
    if (nnz) hipLaunchKernelGGL(k_rev_count, dim3((unsigned)std::min<uint64_t>((nnz + BLOCK - 1) / BLOCK, 8192)), dim3(BLOCK), 0, c->stream,
                                (const int32_t *)c->g.d_col.get(), nnz, indeg.get());
    std::vector<uint32_t> h_in(n);
    HIPCHK(c, hipMemcpyAsync(h_in.data(), indeg.get(), n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int64_t> rp(n + 1);
    rp[0] = 0;
    for (uint64_t v = 0; v < n; v++) rp[v + 1] = rp[v] + h_in[v];
    ReverseCsr rev;
    HIPCHK(c, rev.d_rin_ptr.alloc(n + 1));
    HIPCHK(c, rev.d_rin.alloc(std::max<uint64_t>(1, nnz)));
    HIPCHK(c, cursor.alloc(std::max<uint64_t>(1, n)));
    HIPCHK(c, hipMemcpyAsync(rev.d_rin_ptr.get(), rp.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(cursor.get(), rp.data(), n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rev_fill, dim3((unsigned)std::min<uint64_t>((n * 64 + BLOCK - 1) / BLOCK, 16384)), dim3(BLOCK), 0, c->stream,
                       (const int64_t *)c->g.d_row_ptr.get(), (const int32_t *)c->g.d_col.get(), c->g.n, cursor.get(), rev.d_rin.get());
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the host vectors and the cursor go out of scope)
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, FORA_E_HIP, std::string("reverse CSR: ") + hipGetErrorString(e));
    c->g.rev = std::move(rev);
    return FORA_OK;
}

static int ensure_bwd_targets(fora_ctx *c, uint64_t nt) {
    BwdBufs &b = c->bw;
    const uint64_t m = std::max<uint64_t>(1, nt);
    HIPCHK(c, b.d_bstat.ensure(BS_WORDS));
    if (b.d_boff.size() < m + 1) { b.d_bt.reset(); b.d_bcnt.reset(); b.d_bspill.reset(); b.d_blist.reset(); b.d_bflag.reset(); b.d_boff.reset(); } // a regrow frees the group first: its peak memory
    HIPCHK(c, b.d_bt.ensure(m));
    HIPCHK(c, b.d_bcnt.ensure(m));
    HIPCHK(c, b.d_bspill.ensure(m));
    HIPCHK(c, b.d_blist.ensure(m));
    HIPCHK(c, b.d_bflag.ensure(m));
    HIPCHK(c, b.d_boff.ensure(m + 1));
    return FORA_OK;
}

// global tier: dense slabs for up to 64 targets in flight, 36 bytes per node each, at most a quarter of the free HBM
static int ensure_global_tier(fora_ctx *c) {
    if (c->g.tier.d_gr) return FORA_OK;
    const uint64_t n = (uint64_t)c->g.n;
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    const uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>({64, (uint64_t)c->prop.multiProcessorCount, (uint64_t)(fr / 4) / (36 * n)}));
    GlobalTier t;
    HIPCHK(c, t.d_gr.alloc(g * n));
    HIPCHK(c, t.d_gp.alloc(g * n));
    HIPCHK(c, t.d_gfy.alloc(g * n));
    HIPCHK(c, t.d_gtag.alloc(g * n));
    HIPCHK(c, t.d_glist.alloc(g * n));
    HIPCHK(c, t.d_gfn.alloc(g * n));
    // (on the ctx stream: it does not synchronise with the null stream, and the first global-tier kernel must see zeros)
    HIPCHK(c, t.d_gr.zero(c->stream));
    HIPCHK(c, t.d_gp.zero(c->stream));
    HIPCHK(c, t.d_gtag.zero(c->stream));
    t.wgs = (uint32_t)g;
    c->g.tier = std::move(t);
    return FORA_OK;
}

struct BwdRun {
    uint64_t thr = 0, afix = 0;
    uint32_t cap = 0;
    std::vector<uint32_t> cnt;   // entries per target
    std::vector<uint32_t> spill; // targets of the global tier, ascending
    std::vector<uint64_t> off;   // first entry of target i over the whole call (nt + 1)
    std::vector<std::pair<uint32_t, uint32_t>> chunks; // [t0, t1)
    uint64_t stat[BS_WORDS] = {};
};

static BwdDev make_bwd(fora_ctx *c, const BwdRun &r) {
    BwdDev b{};
    b.rin_ptr = c->g.rev.d_rin_ptr.get(); b.rin = c->g.rev.d_rin.get(); b.deg = c->g.d_deg.get();
    b.targets = c->bw.d_bt.get(); b.cap = r.cap; b.thr = r.thr; b.afix = r.afix;
    b.cnt = c->bw.d_bcnt.get(); b.spilled = c->bw.d_bflag.get(); b.spill = c->bw.d_bspill.get(); b.stat = c->bw.d_bstat.get();
    b.off = c->bw.d_boff.get(); b.e_node = c->bw.d_enode.get(); b.e_p = c->bw.d_ep.get(); b.e_r = c->bw.d_er.get();
    b.g_r = c->g.tier.d_gr.get(); b.g_p = c->g.tier.d_gp.get(); b.g_fy = c->g.tier.d_gfy.get(); b.g_tag = c->g.tier.d_gtag.get(); b.g_list = c->g.tier.d_glist.get(); b.g_fn = c->g.tier.d_gfn.get();
    b.n = (uint32_t)c->g.n;
    b.err = (uint32_t *)(c->bw.d_bstat.get() + BS_WORDS - 1);
    return b;
}

static unsigned bwd_grid(const fora_ctx *c, uint64_t items, uint64_t per_cu) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(items, (uint64_t)c->prop.multiProcessorCount * per_cu));
}

static int bwd_check_err(fora_ctx *c, const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, FORA_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return FORA_OK;
}

// count pass over the nt targets already in d_bt; then the chunks
static int bwd_count(fora_ctx *c, uint32_t nt, double rmax, BwdRun &r) {
    r.thr = (uint64_t)std::floor(std::ldexp(rmax, 60));
    r.afix = (uint64_t)std::ldexp(c->par.alpha, 62); // (as the forward push: make_dev's afix)
    r.cap = (uint32_t)std::min<int64_t>(std::max<int64_t>(c->opt_.bwd_lds_cap, 0), BWD_CAP_MAX);
    HIPCHK(c, hipMemsetAsync(c->bw.d_bstat.get(), 0, BS_WORDS * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->bw.d_bflag.get(), 0, nt, c->stream));
    EvSpan ev(c, EV_BWD);
    if (r.cap > 0) {
        BwdDev b = make_bwd(c, r);
        b.nlist = nt;
        hipLaunchKernelGGL((k_bwd_push<false, false>), dim3(bwd_grid(c, nt, 8)), dim3(BLOCK), 0, c->stream, b);
    }
    HIPCHK(c, hipMemcpyAsync(r.stat, c->bw.d_bstat.get(), BS_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (r.cap > 0) {
        r.spill.resize(r.stat[BS_SPILL]);
        if (!r.spill.empty()) {
            HIPCHK(c, hipMemcpy(r.spill.data(), c->bw.d_bspill.get(), r.spill.size() * 4, hipMemcpyDeviceToHost));
            std::sort(r.spill.begin(), r.spill.end());
        }
    } else {
        r.spill.resize(nt);
        for (uint32_t i = 0; i < nt; i++) r.spill[i] = i;
    }
    if (!r.spill.empty()) {
        if (int rc = ensure_global_tier(c)) return rc;
        HIPCHK(c, hipMemcpyAsync(c->bw.d_blist.get(), r.spill.data(), r.spill.size() * 4, hipMemcpyHostToDevice, c->stream));
        BwdDev b = make_bwd(c, r);
        b.list = c->bw.d_blist.get();
        b.nlist = (uint32_t)r.spill.size();
        hipLaunchKernelGGL((k_bwd_push<true, false>), dim3(std::min<uint32_t>(c->g.tier.wgs, b.nlist)), dim3(BLOCK), 0, c->stream, b);
    }
    ev.end();
    r.cnt.resize(nt);
    HIPCHK(c, hipMemcpyAsync(r.cnt.data(), c->bw.d_bcnt.get(), (size_t)nt * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(r.stat, c->bw.d_bstat.get(), BS_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = bwd_check_err(c, "backward push")) return rc;
    if (r.stat[BS_WORDS - 1] & 0xFFFFFFFFull) return fail(c, FORA_E_OVERFLOW, "backward push: level cap reached");
    r.off.assign((size_t)nt + 1, 0);
    for (uint32_t i = 0; i < nt; i++) r.off[i + 1] = r.off[i] + r.cnt[i];
    // chunks: at most bwd_chunk targets, at most the entries a fifth of the free HBM holds (20 bytes each)
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    const uint64_t have = std::min({c->bw.d_enode.size(), c->bw.d_ep.size(), c->bw.d_er.size()});
    const uint64_t budget = std::max<uint64_t>({have, (uint64_t)(fr / 5) / 20, (uint64_t)BWD_CAP_MAX});
    const uint64_t per = c->opt_.bwd_chunk > 0 ? (uint64_t)c->opt_.bwd_chunk : ~0ull;
    r.chunks.clear();
    for (uint32_t t0 = 0; t0 < nt;) {
        uint32_t t1 = t0 + 1; // (one target always fits: a global-tier target has at most n entries, see the budget check below)
        while (t1 < nt && t1 - t0 < per && r.off[t1 + 1] - r.off[t0] <= budget) t1++;
        r.chunks.push_back({t0, t1});
        t0 = t1;
    }
    return FORA_OK;
}

// write pass of chunk k: entries of its targets into d_enode / d_ep / d_er, offsets d_boff (chunk-relative)
static int bwd_write(fora_ctx *c, const BwdRun &r, size_t k) {
    const uint32_t t0 = r.chunks[k].first, t1 = r.chunks[k].second, len = t1 - t0;
    const uint64_t ne = r.off[t1] - r.off[t0];
    if (c->bw.d_er.size() < ne) { c->bw.d_enode.reset(); c->bw.d_ep.reset(); c->bw.d_er.reset(); } // (as ensure_bwd_targets)
    HIPCHK(c, c->bw.d_enode.ensure(ne));
    HIPCHK(c, c->bw.d_ep.ensure(ne));
    HIPCHK(c, c->bw.d_er.ensure(ne));
    std::vector<uint64_t> off((size_t)len + 1);
    for (uint32_t i = 0; i <= len; i++) off[i] = r.off[t0 + i] - r.off[t0];
    std::vector<uint32_t> gl;
    for (auto it = std::lower_bound(r.spill.begin(), r.spill.end(), t0); it != r.spill.end() && *it < t1; ++it) gl.push_back(*it - t0);
    HIPCHK(c, hipMemcpyAsync(c->bw.d_boff.get(), off.data(), off.size() * 8, hipMemcpyHostToDevice, c->stream));
    if (!gl.empty()) HIPCHK(c, hipMemcpyAsync(c->bw.d_blist.get(), gl.data(), gl.size() * 4, hipMemcpyHostToDevice, c->stream));
    EvSpan ev(c, EV_BWD);
    BwdDev b = make_bwd(c, r);
    b.targets = c->bw.d_bt.get() + t0;
    b.spilled = c->bw.d_bflag.get() + t0;
    if (r.cap > 0 && gl.size() < len) {
        b.nlist = len;
        hipLaunchKernelGGL((k_bwd_push<false, true>), dim3(bwd_grid(c, len, 8)), dim3(BLOCK), 0, c->stream, b);
    }
    if (!gl.empty()) {
        b.list = c->bw.d_blist.get();
        b.nlist = (uint32_t)gl.size();
        hipLaunchKernelGGL((k_bwd_push<true, true>), dim3(std::min<uint32_t>(c->g.tier.wgs, b.nlist)), dim3(BLOCK), 0, c->stream, b);
    }
    ev.end();
    uint64_t st[BS_WORDS];
    HIPCHK(c, hipMemcpyAsync(st, c->bw.d_bstat.get(), sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (off / gl are host vectors of this frame)
    if (int rc = bwd_check_err(c, "backward push (write)")) return rc;
    if (st[BS_WORDS - 1] & 0xFFFFFFFFull) {
        const uint64_t i = st[BS_BAD] ? st[BS_BAD] - 1 + t0 : 0;
        char buf[200];
        snprintf(buf, sizeof(buf), "backward push: write pass disagrees with its count pass (target index %llu, %u entries counted, %s tier)",
                 (unsigned long long)i, st[BS_BAD] ? r.cnt[i] : 0u, std::binary_search(r.spill.begin(), r.spill.end(), (uint32_t)i) ? "global" : "LDS");
        return fail(c, FORA_E_OVERFLOW, buf);
    }
    return FORA_OK;
}

static int check_bwd_rmax(fora_ctx *c, double rmax) {
    if (!(rmax > 0) || !std::isfinite(rmax)) return fail(c, FORA_E_ARG, "rmax must be > 0");
    // every residue stays below max(1, rmax / alpha) and every estimate below 1 + that: u64 at 2^60 holds less than 16
    if (!(1.0 + std::max(1.0, rmax / c->par.alpha) < 16.0)) return fail(c, FORA_E_ARG, "rmax / alpha too large for the 2^60 fixed point");
    return FORA_OK;
}

static void fill_bwd_stats(fora_ctx *c, const BwdRun &r, uint64_t nt, fora_bwd_stats *bwd, double walk_ms) {
    if (!bwd) return;
    memset(bwd, 0, sizeof(*bwd));
    bwd->targets = nt;
    bwd->pops = r.stat[BS_POPS];
    bwd->relax = r.stat[BS_RELAX];
    bwd->entries = r.stat[BS_ENTRIES];
    bwd->global_targets = r.spill.size();
    bwd->levels = (int32_t)r.stat[BS_LEVELS];
    bwd->chunks = (int32_t)r.chunks.size();
    bwd->bwd_ms = c->tm.bwd_ms;
    bwd->walk_ms = walk_ms;
    bwd->combine_ms = c->tm.combine_ms;
}

static int bwdpush_batch_impl(fora_ctx *c, const int32_t *targets, int nt, double rmax, uint64_t *reserve_fix_out,
                              uint64_t *residue_fix_out, fora_bwd_stats *bwd) {
    if (int rc = check_batch_args(c, targets, nt, "target")) return rc;
    if (int rc = check_id_range(c, targets, nt, "target")) return rc;
    if (int rc = check_bwd_rmax(c, rmax)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    c->tm.bwd_ms = c->tm.combine_ms = 0;
    BwdRun r;
    if (nt == 0) { fill_bwd_stats(c, r, 0, bwd, 0); return FORA_OK; }
    if (int rc = ensure_reverse_csr(c)) return rc;
    if (int rc = ensure_bwd_targets(c, (uint64_t)nt)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->bw.d_bt.get(), targets, (size_t)nt * 4, hipMemcpyHostToDevice, c->stream));
    if (int rc = bwd_count(c, (uint32_t)nt, rmax, r)) return rc;
    const uint64_t n = (uint64_t)c->g.n;
    if (reserve_fix_out) memset(reserve_fix_out, 0, (size_t)nt * n * 8);
    if (residue_fix_out) memset(residue_fix_out, 0, (size_t)nt * n * 8);
    for (size_t k = 0; k < r.chunks.size() && (reserve_fix_out || residue_fix_out); k++) {
        if (int rc = bwd_write(c, r, k)) return rc;
        const uint32_t t0 = r.chunks[k].first, t1 = r.chunks[k].second;
        const uint64_t ne = r.off[t1] - r.off[t0];
        std::vector<uint32_t> nd(ne);
        std::vector<uint64_t> p(ne), q(ne);
        HIPCHK(c, hipMemcpy(nd.data(), c->bw.d_enode.get(), ne * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(p.data(), c->bw.d_ep.get(), ne * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(q.data(), c->bw.d_er.get(), ne * 8, hipMemcpyDeviceToHost));
        for (uint32_t i = t0; i < t1; i++)
            for (uint64_t e = r.off[i] - r.off[t0]; e < r.off[i + 1] - r.off[t0]; e++) {
                if (reserve_fix_out) reserve_fix_out[(uint64_t)i * n + nd[e]] = p[e];
                if (residue_fix_out) residue_fix_out[(uint64_t)i * n + nd[e]] = q[e];
            }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ev_collect(c);
    fill_bwd_stats(c, r, (uint64_t)nt, bwd, 0);
    return FORA_OK;
}

// ---- Monte-Carlo (--algo montecarlo) and BiPPR: one batch loop of walks.  Monte-Carlo: W walks per source (k_walk_mc),
// omega = montecarlo_setting (algo.h:477-483).  BiPPR: the same walks at bippr_setting's omega, combined with the backward
// push's entries of every node (bippr_query, query.h:71-124).
// W = the integers i >= 0 with i < omega (for (unsigned long i = 0; i < config.omega; i++)), walk j carrying wbase + (j < wrem)
// units of FIX_ONE
struct WalkCount { uint64_t W = 0, wbase = 0, wrem = 0; };
static int walk_count(fora_ctx *c, double omega, WalkCount &w) {
    if (!(omega < 0x1p48)) return fail(c, FORA_E_ARG, "epsilon too small: more than 2^48 walks per source");
    w.W = (uint64_t)std::ceil(omega);
    if (w.W == 0) return fail(c, FORA_E_ARG, "no walks");
    w.wbase = FIX_ONE / w.W;
    w.wrem = FIX_ONE % w.W;
    return FORA_OK;
}

// A launch runs at most MC_LAUNCH_WALKS walks over all slots of the batch.
constexpr uint64_t MC_LAUNCH_WALKS = 1ull << 28;
// walks j < W of every slot of the batch (k_walk_mc) into the slots' ppr slabs
static void launch_mc_walks(fora_ctx *c, const Dev &d, int nb, const WalkCount &w) {
    // walk numbers per launch and per workgroup: about eight workgroups per CU, 4 Ki .. 64 Ki walks each
    const uint64_t span = std::max<uint64_t>(1, MC_LAUNCH_WALKS / (uint64_t)nb);
    for (uint64_t j0 = 0; j0 < w.W; j0 += span) {
        const uint64_t j1 = std::min(w.W, j0 + span);
        const uint64_t wgs = std::max<uint64_t>(1, (uint64_t)c->prop.multiProcessorCount * 8 / (uint64_t)nb);
        const uint64_t per_wg = std::min<uint64_t>(1 << 16, std::max<uint64_t>(1 << 12, (j1 - j0 + wgs - 1) / wgs));
        const unsigned X = (unsigned)((j1 - j0 + per_wg - 1) / per_wg);
        EvSpan ev(c, EV_WALK);
        hipLaunchKernelGGL(k_walk_mc, dim3(X, nb), dim3(BLOCK), 0, c->stream, d, w.wbase, w.wrem, j0, j1, per_wg);
    }
}

// BiPPR's step of a batch: the walk slabs c_b (2^-62, slot-major in d_ppr) -> node-major in the residue slabs, combined with
// the entries of every chunk of targets into d_ppr, -> slot-major estimates at 2^-60 in the residue slabs
static int bippr_combine(fora_ctx *c, const BwdRun &r, int nb) {
    const uint64_t n = (uint64_t)c->g.n;
    const uint64_t tiles = ((uint64_t)nb + 31) / 32 * ((n + 31) / 32);
    EvSpan ev(c, EV_COMBINE);
    hipLaunchKernelGGL(k_transpose_u64, dim3((unsigned)tiles), dim3(BLOCK), 0, c->stream, (const uint64_t *)c->ws.d_ppr.get(), c->ws.d_residue.get(),
                       (uint64_t)nb, n); // -> node-major [n][nb] in the residue slabs
    ev.end();
    const bool one_chunk = r.chunks.size() == 1; // (then its entries were written once for every batch)
    for (size_t ck = 0; ck < r.chunks.size(); ck++) {
        if (!one_chunk) if (int rc = bwd_write(c, r, ck)) return rc;
        const uint32_t t0 = r.chunks[ck].first, len = r.chunks[ck].second - t0;
        ev.begin(EV_COMBINE);
        hipLaunchKernelGGL(k_bippr_combine, dim3((unsigned)(((uint64_t)len * 64 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream,
                           (const uint64_t *)c->ws.d_residue.get(), (uint32_t)nb, (const int32_t *)c->ws.d_src.get(), (const uint64_t *)c->bw.d_boff.get(),
                           (const uint32_t *)c->bw.d_enode.get(), (const uint64_t *)c->bw.d_ep.get(), (const uint64_t *)c->bw.d_er.get(), t0, len, c->ws.d_ppr.get());
        ev.end();
    }
    ev.begin(EV_COMBINE);
    hipLaunchKernelGGL(k_transpose_u64, dim3((unsigned)tiles), dim3(BLOCK), 0, c->stream, (const uint64_t *)c->ws.d_ppr.get(), c->ws.d_residue.get(),
                       n, (uint64_t)nb); // -> slot-major estimates at 2^-60 in the residue slabs
    return FORA_OK;
}

// The batch loop: walks into the ppr slabs, BiPPR's combine when `bwd` holds the backward push of the call, then k_ppr_sum,
// top-k, stats and copy-out of the estimates (Monte-Carlo: the ppr slabs at 2^-62; BiPPR: the residue slabs at 2^-60).
static int walk_batches(fora_ctx *c, const int32_t *sources, int nq, const WalkCount &w, const BwdRun *bwd, double rmax_used,
                        double *ppr_out, uint64_t *ppr_fix_out, int k, int32_t *ids, double *scores, fora_query_stats *stats) {
    const bool want_topk = k > 0 && (ids || scores);
    uint64_t *const est = bwd ? c->ws.d_residue.get() : c->ws.d_ppr.get();
    const int frac = bwd ? 60 : 62;
    const int per = even_batch(nq, c->ws.B);
    for (int b0 = 0; b0 < nq; b0 += per) {
        const int nb = std::min(per, nq - b0);
        EvSpan batch(c, EV_BATCH);
        int rc = reset_batch_state(c, nb, sources + b0);
        if (rc) return rc;
        HIPCHK(c, c->ws.d_qs.zero(c->stream, (size_t)nb));
        const Dev d = make_dev(c, nb, false);
        launch_mc_walks(c, d, nb, w);
        if (bwd && (rc = bippr_combine(c, *bwd, nb))) return rc;
        Dev de = d;
        de.ppr = est;
        {
            const uint32_t chunks = (uint32_t)std::min<int64_t>(((int64_t)c->g.n + BLOCK - 1) / BLOCK, 64);
            EvSpan ev(c, EV_OTHER);
            hipLaunchKernelGGL(k_ppr_sum, dim3(chunks, nb), dim3(BLOCK), 0, c->stream, de);
        }
        if (want_topk) {
            EvSpan ev(c, EV_OTHER);
            if ((rc = launch_select(c, de, nb, k, c->ws.d_topk_ids.get(), c->ws.d_topk_sc.get(), 0))) return rc;
        }
        HIPCHK(c, hipMemcpyAsync(c->ws.h_qs_pin.get(), c->ws.d_qs.get(), (size_t)nb * sizeof(QState), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->ws.h_steps_pin.get(), d.tot_steps, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        if ((rc = close_batch(c, &batch, bwd ? "bippr" : "montecarlo"))) return rc;
        c->tm.total.walks += w.W * (uint64_t)nb;
        c->tm.total.walk_steps += *c->ws.h_steps_pin.get();
        if (stats)
            for (int i = 0; i < nb; i++) {
                fora_query_stats &o = stats[b0 + i];
                memset(&o, 0, sizeof(o));
                o.n_walks = w.W;
                o.rmax_used = rmax_used;
                o.ppr_sum_fix = c->ws.h_qs_pin.get()[i].ppr_sum;
                o.dangling_source = is_dangling(c, sources[b0 + i]) ? 1 : 0;
            }
        // (k_topk_select scales by 2^-62: BiPPR's scores x 4)
        if (want_topk && (rc = copy_topk_out(c, nb, k, ids, scores, (uint64_t)b0, nullptr, bwd ? 4.0 : 1.0))) return rc;
        if ((rc = copy_slab_out(c, est, 0, (uint64_t)b0, (uint64_t)nb, ppr_fix_out, ppr_out, frac))) return rc;
    }
    return FORA_OK;
}

static int montecarlo_batch_impl(fora_ctx *c, const int32_t *sources, int nq, double epsilon, double *ppr_out,
                                 uint64_t *ppr_fix_out, int k, int32_t *ids, double *scores, fora_query_stats *stats) {
    if (int rc = check_baseline_args(c, sources, nq, epsilon, k)) return rc;
    const double delta = 1.0 / c->g.n, pfail = 1.0 / c->g.n;
    WalkCount w;
    if (int rc = walk_count(c, 3 * log(2 / pfail) / epsilon / epsilon / delta, w)) return rc; // fwd_rw_count, algo.h:478
    HIPCHK(c, hipSetDevice(c->device));
    // (the FORA plan: only the ppr slabs and the per-slot words are used here)
    if (int rc = ensure_query_workspace(c, nq, k > 0 && (ids || scores) ? k : 0)) return rc;
    return walk_batches(c, sources, nq, w, nullptr, 0, ppr_out, ppr_fix_out, k, ids, scores, stats);
}

static int bippr_batch_impl(fora_ctx *c, const int32_t *sources, int nq, double epsilon, double rmax_scale, double *ppr_out,
                            uint64_t *ppr_fix_out, int k, int32_t *ids, double *scores, fora_query_stats *stats, fora_bwd_stats *bwd) {
    if (int rc = check_baseline_args(c, sources, nq, epsilon, k)) return rc;
    if (c->g.m_attr <= 0) return fail(c, FORA_E_ARG, "m of the graph must be > 0");
    if (!(rmax_scale > 0) || !std::isfinite(rmax_scale)) return fail(c, FORA_E_ARG, "rmax_scale must be > 0");
    const double delta = 1.0 / c->g.n, pfail = 1.0 / c->g.n;
    double rmax = epsilon * sqrt(c->g.m_attr * 1.0 * delta / 3.0 / log(2.0 / pfail)); // bippr_setting, algo.h:442-447
    rmax *= rmax_scale;
    const double omega = rmax * 3 * log(2.0 / pfail) / delta / epsilon / epsilon;
    if (int rc = check_bwd_rmax(c, rmax)) return rc;
    WalkCount w;
    if (int rc = walk_count(c, omega, w)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    c->tm.bwd_ms = c->tm.combine_ms = 0;
    const double walk_ms0 = c->tm.total.walk_ms;
    BwdRun r;
    if (nq == 0) { fill_bwd_stats(c, r, 0, bwd, 0); return FORA_OK; }
    // (the FORA plan: the ppr and residue slabs and the per-slot words are used here)
    int rc = ensure_query_workspace(c, nq, k > 0 && (ids || scores) ? k : 0);
    if (rc) return rc;
    const uint64_t n = (uint64_t)c->g.n;
    // every node is a target (query.h:91: for i < graph.n)
    if ((rc = ensure_reverse_csr(c))) return rc;
    if ((rc = ensure_bwd_targets(c, n))) return rc;
    {
        std::vector<int32_t> iota(n);
        for (uint64_t v = 0; v < n; v++) iota[v] = (int32_t)v;
        HIPCHK(c, hipMemcpyAsync(c->bw.d_bt.get(), iota.data(), n * 4, hipMemcpyHostToDevice, c->stream));
        if ((rc = bwd_count(c, (uint32_t)n, rmax, r))) return rc; // (synchronises)
    }
    if (r.chunks.size() == 1 && (rc = bwd_write(c, r, 0))) return rc; // shared by every batch
    if ((rc = walk_batches(c, sources, nq, w, &r, rmax, ppr_out, ppr_fix_out, k, ids, scores, stats))) return rc;
    fill_bwd_stats(c, r, n, bwd, c->tm.total.walk_ms - walk_ms0);
    return FORA_OK;
}

// ---- targeted BiPPR: the estimate of bippr_batch_impl for a caller's list of targets, nt backward pushes instead of n
// (the TARGETED BIPPR contract of include/fora_hip.h).
// Lane mapping of k_bippr_combine_targets for a batch of nb slots and a call of `entries` entries.  Lane = slot reads
// 8 nb contiguous bytes per entry but needs the slabs transposed first (16 n nb bytes); lane = entry gathers one word per
// lane from the slot-major slabs, a 64-byte sector for 8 bytes.  So: by entry while fewer than 16 slots would leave three
// quarters of a wave idle, and while the gathers' 64 nb E bytes stay under the transpose's 16 n nb, E < n / 4.
static bool want_by_slot(const fora_ctx *c, int nb, uint64_t entries) {
    if (c->opt_.tgt_lanes >= 0) return c->opt_.tgt_lanes == 0;
    return nb >= 16 && entries >= (uint64_t)c->g.n / 4;
}

// The combine of a batch: the walk slabs of the nb slots (slot-major in d_ppr) with the entries of every chunk into the
// zeroed block `out` ([nb][nt]).
static int bippr_combine_targets(fora_ctx *c, const BwdRun &r, int nb, uint64_t nt, unsigned long long *out) {
    const uint64_t n = (uint64_t)c->g.n;
    const bool by_slot = want_by_slot(c, nb, r.off[nt]);
    if (by_slot) {
        EvSpan ev(c, EV_COMBINE);
        hipLaunchKernelGGL(k_transpose_u64, dim3((unsigned)(((uint64_t)nb + 31) / 32 * ((n + 31) / 32))), dim3(BLOCK), 0, c->stream,
                           (const uint64_t *)c->ws.d_ppr.get(), c->ws.d_residue.get(), (uint64_t)nb, n); // -> node-major [n][nb] in the residue slabs
    }
    const uint64_t *slabs = by_slot ? c->ws.d_residue.get() : c->ws.d_ppr.get();
    const uint64_t groups = by_slot ? ((uint64_t)nb + 63) / 64 : 1;
    const bool one_chunk = r.chunks.size() == 1; // (then its entries were written once for every batch)
    for (size_t ck = 0; ck < r.chunks.size(); ck++) {
        if (!one_chunk) if (int rc = bwd_write(c, r, ck)) return rc;
        const uint32_t t0 = r.chunks[ck].first, t1 = r.chunks[ck].second;
        const uint64_t ne = r.off[t1] - r.off[t0];
        if (!ne) continue;
        // entries per wave: about 32 waves per CU over the launch, 64 .. 1024 entries each
        uint64_t span = c->opt_.tgt_span > 0 ? (uint64_t)c->opt_.tgt_span
                                             : std::min<uint64_t>(1024, std::max<uint64_t>(64, ne * groups / ((uint64_t)c->prop.multiProcessorCount * 32)));
        span = std::min<uint64_t>(span, 1u << 30);
        const uint64_t waves = (ne + span - 1) / span;
        const dim3 grid((unsigned)((waves + BLOCK / 64 - 1) / (BLOCK / 64)), (unsigned)groups);
        EvSpan ev(c, EV_COMBINE);
        if (by_slot)
            hipLaunchKernelGGL((k_bippr_combine_targets<true>), grid, dim3(BLOCK), 0, c->stream, slabs, (uint32_t)nb, n, (const int32_t *)c->ws.d_src.get(),
                               (const uint64_t *)c->bw.d_boff.get(), (const uint32_t *)c->bw.d_enode.get(), (const uint64_t *)c->bw.d_ep.get(), (const uint64_t *)c->bw.d_er.get(), t0,
                               t1 - t0, (uint32_t)span, nt, out);
        else
            hipLaunchKernelGGL((k_bippr_combine_targets<false>), grid, dim3(BLOCK), 0, c->stream, slabs, (uint32_t)nb, n, (const int32_t *)c->ws.d_src.get(),
                               (const uint64_t *)c->bw.d_boff.get(), (const uint32_t *)c->bw.d_enode.get(), (const uint64_t *)c->bw.d_ep.get(), (const uint64_t *)c->bw.d_er.get(), t0,
                               t1 - t0, (uint32_t)span, nt, out);
    }
    return FORA_OK;
}

static int bippr_targets_batch_impl(fora_ctx *c, const int32_t *sources, int nq, const int32_t *targets, int nt, double epsilon,
                                    double rmax_scale, double *est_out, uint64_t *est_fix_out, fora_query_stats *stats,
                                    fora_bwd_stats *bwd) {
    if (int rc = check_batch_args(c, sources, nq)) return rc;
    if (int rc = check_batch_args(c, targets, nt, "target")) return rc;
    if (!(epsilon > 0)) return fail(c, FORA_E_ARG, "epsilon must be > 0");
    if (c->g.m_attr <= 0) return fail(c, FORA_E_ARG, "m of the graph must be > 0");
    if (!(rmax_scale > 0) || !std::isfinite(rmax_scale)) return fail(c, FORA_E_ARG, "rmax_scale must be > 0");
    const double delta = 1.0 / c->g.n, pfail = 1.0 / c->g.n;
    double rmax = epsilon * sqrt(c->g.m_attr * 1.0 * delta / 3.0 / log(2.0 / pfail)); // bippr_setting, as bippr_batch_impl
    rmax *= rmax_scale;
    const double omega = rmax * 3 * log(2.0 / pfail) / delta / epsilon / epsilon;
    if (int rc = check_bwd_rmax(c, rmax)) return rc;
    WalkCount w;
    if (int rc = walk_count(c, omega, w)) return rc;
    if (int rc = check_id_range(c, sources, nq)) return rc;
    if (int rc = check_id_range(c, targets, nt, "target")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    c->tm.bwd_ms = c->tm.combine_ms = 0;
    const double walk_ms0 = c->tm.total.walk_ms;
    BwdRun r;
    auto fill_stats = [&](int i, uint64_t sum) {
        if (!stats) return;
        fora_query_stats &o = stats[i];
        memset(&o, 0, sizeof(o));
        o.n_walks = w.W;
        o.rmax_used = rmax;
        o.ppr_sum_fix = sum;
        o.dangling_source = is_dangling(c, sources[i]) ? 1 : 0;
    };
    if (nq == 0 || nt == 0) { // nothing to estimate: no push, no walk
        for (int i = 0; i < nq; i++) fill_stats(i, 0);
        fill_bwd_stats(c, r, 0, bwd, 0);
        return FORA_OK;
    }
    // (the FORA plan: the ppr and residue slabs and the per-slot words are used here)
    int rc = ensure_query_workspace(c, nq, 0);
    if (rc) return rc;
    const uint64_t T = (uint64_t)nt;
    const int per = even_batch(nq, c->ws.B);
    // the estimate block of a batch and its row sums
    const size_t words = (size_t)per * (T + 1);
    if (c->bw.d_tgt_est.ensure(words) != hipSuccess || (est_out && c->bw.d_tgt_f64.ensure((size_t)per * T) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(c, FORA_E_NOMEM, "no device memory for the estimate block");
    }
    if ((rc = ensure_reverse_csr(c))) return rc;
    if ((rc = ensure_bwd_targets(c, T))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->bw.d_bt.get(), targets, T * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = bwd_count(c, (uint32_t)nt, rmax, r))) return rc; // (synchronises)
    if (r.chunks.size() == 1 && (rc = bwd_write(c, r, 0))) return rc; // shared by every batch
    std::vector<uint64_t> sums((size_t)per);
    for (int b0 = 0; b0 < nq; b0 += per) {
        const int nb = std::min(per, nq - b0);
        const uint64_t cells = (uint64_t)nb * T;
        EvSpan batch(c, EV_BATCH);
        if ((rc = reset_batch_state(c, nb, sources + b0))) return rc;
        HIPCHK(c, c->bw.d_tgt_est.zero(c->stream, cells + (uint64_t)nb));
        const Dev d = make_dev(c, nb, false);
        launch_mc_walks(c, d, nb, w);
        unsigned long long *const est = (unsigned long long *)c->bw.d_tgt_est.get();
        if ((rc = bippr_combine_targets(c, r, nb, T, est))) return rc;
        {
            EvSpan ev(c, EV_COMBINE);
            hipLaunchKernelGGL(k_bippr_targets_finish, dim3((unsigned)std::min<uint64_t>((T + BLOCK - 1) / BLOCK, 64), (unsigned)nb), dim3(BLOCK), 0,
                               c->stream, (const uint64_t *)c->bw.d_tgt_est.get(), T, est_out ? c->bw.d_tgt_f64.get() : nullptr, est + cells);
        }
        HIPCHK(c, hipMemcpyAsync(c->ws.h_steps_pin.get(), d.tot_steps, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        if ((rc = close_batch(c, &batch, "bippr targets"))) return rc;
        c->tm.total.walks += w.W * (uint64_t)nb;
        c->tm.total.walk_steps += *c->ws.h_steps_pin.get();
        if (stats) {
            HIPCHK(c, hipMemcpy(sums.data(), c->bw.d_tgt_est.get() + cells, (size_t)nb * 8, hipMemcpyDeviceToHost));
            for (int i = 0; i < nb; i++) fill_stats(b0 + i, sums[(size_t)i]);
        }
        if (est_fix_out) HIPCHK(c, hipMemcpy(est_fix_out + (uint64_t)b0 * T, c->bw.d_tgt_est.get(), cells * 8, hipMemcpyDeviceToHost));
        if (est_out) HIPCHK(c, hipMemcpy(est_out + (uint64_t)b0 * T, c->bw.d_tgt_f64.get(), cells * 8, hipMemcpyDeviceToHost));
    }
    fill_bwd_stats(c, r, T, bwd, c->tm.total.walk_ms - walk_ms0);
    return FORA_OK;
}

int fora_hip_montecarlo_batch(fora_ctx *c, const int32_t *sources, int nq, double epsilon, double *ppr_out, uint64_t *ppr_fix_out,
                              int k, int32_t *ids, double *scores, fora_query_stats *stats) {
    return drop_pairs_unless_ok(c, montecarlo_batch_impl(c, sources, nq, epsilon, ppr_out, ppr_fix_out, k, ids, scores, stats)); // (no buckets, no push: nothing to retry)
}

int fora_hip_bwdpush_batch(fora_ctx *c, const int32_t *targets, int nt, double rmax, uint64_t *reserve_fix_out,
                           uint64_t *residue_fix_out, fora_bwd_stats *bwd) {
    return drop_pairs_unless_ok(c, bwdpush_batch_impl(c, targets, nt, rmax, reserve_fix_out, residue_fix_out, bwd));
}

int fora_hip_bippr_batch(fora_ctx *c, const int32_t *sources, int nq, double epsilon, double rmax_scale, double *ppr_out,
                         uint64_t *ppr_fix_out, int k, int32_t *ids, double *scores, fora_query_stats *stats, fora_bwd_stats *bwd) {
    return drop_pairs_unless_ok(c, bippr_batch_impl(c, sources, nq, epsilon, rmax_scale, ppr_out, ppr_fix_out, k, ids, scores, stats, bwd));
}

int fora_hip_bippr_targets_batch(fora_ctx *c, const int32_t *sources, int nq, const int32_t *targets, int nt, double epsilon,
                                 double rmax_scale, double *est_out, uint64_t *est_fix_out, fora_query_stats *stats, fora_bwd_stats *bwd) {
    return drop_pairs_unless_ok(c, bippr_targets_batch_impl(c, sources, nq, targets, nt, epsilon, rmax_scale, est_out, est_fix_out, stats, bwd));
}

int fora_hip_reset_timing(fora_ctx *c) {
    if (!c) return FORA_E_ARG;
    c->tm.total = fora_timing{};
    (void)hipSetDevice(c->device);
    (void)hipMemset(c->d_stamps.get(), 0, 32 * sizeof(unsigned long long));
    return FORA_OK;
}
int fora_hip_get_stamps(fora_ctx *c, uint64_t *out32) {
    if (!c || !out32) return FORA_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(out32, c->d_stamps.get(), 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return FORA_OK;
}
int fora_hip_get_timing(fora_ctx *c, fora_timing *out) {
    if (!c || !out) return FORA_E_ARG;
    *out = c->tm.total;
    return FORA_OK;
}

} // extern "C"
