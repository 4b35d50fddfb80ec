// engine.hip — the MI355X (gfx950) BFS engine behind include/tlamc.h: the HOST half (Engine: buffers, streams, the level loop of a fused
// run, the step calls of a sharded one, checkpoints, the C ABI); the kernels it launches are in engine_kernels.h.
//
// Per BFS level the frontier (a contiguous index range of the state arena in HBM) is processed in chunks of `chunk_states`
// (bench.py: 2^23) with no host synchronisation inside a level; the host reads one small counter block per level, and while
// levels are small it enqueues eight of them blind (LevelCtl).  The kernels, in the order they matter:
//
//   k_expand_family<Spec, ROUTE>   (specs with action families: raft)  one wavefront = one arena block of 64 parents, one
//                       workgroup = two (MC_EXPAND_WAVES; four until round 5).  Guards -> enabled (parent, slot) pairs, dense slots and the actions of in-flight
//                       messages evaluated by the parent's lane, the sparse fixed slots bucketed per family in LDS and evaluated
//                       64 pairs of ONE family at a time; successors that can never be stored are counted, not evaluated
//                       (S::GENERATED_ONLY); a candidate's fingerprint is the parent's plus O(delta) terms; a per-wavefront
//                       filter drops repeats; 64 candidates at a time probe the seen-set (open addressing over 32- or 64-byte
//                       buckets in HBM, agent-scope atomicCAS on write-once slots).  ROUTE = false (fused runs): the
//                       survivors wait in LDS and the WORKGROUP (a pair of wavefronts) writes them at its end — pooled, counting-sorted by action
//                       class, one atomicAdd on the arena's fill level, row copy + patch from the parent's Summary (the
//                       in-wave tail; wave_write_survivors).  ROUTE = true (sharded runs): candidates of other owners go to
//                       exchange buckets, the rank's own are probed here and go through the new-list.
//   k_expand_insert<Spec, ROUTE>   the slot-by-slot form of the same (lane = parent, loop = action slot; every other spec).
//   k_materialise<Spec> one lane per entry of the new-list (the survivors a wavefront had no list space for, every survivor of
//                       a spec without in-wave writes, of a fast-growing level, or of a sharded run): re-evaluates its
//                       (parent, slot) and writes the full successor (coalesced: consecutive lanes own consecutive arena
//                       indices), plus (parent, slot) for counterexamples.  Runs on a second stream beside the next expand.
//   k_expand + k_insert the round-1 form — a slot-major candidate matrix between two kernels — kept behind MC_F_MATRIX for A/B.
//
// Algorithmic HBM bytes per distinct state = 2*W + 8*(G/D)  (SURVEY.md §8d): each state is written once and read once, each
// in-model successor touches one seen-set word; DESIGN.md §5 has what the kernels really move and what bounds them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <type_traits>
#include <string>
#include <vector>

#include "spec_registry.h"
#include "hip_owned.h"        // DevBuf, PinnedBuf, Event, Stream: every HIP resource of the host half is held by one of these; HIP_TRY, set_error

namespace mc {

// The library is built from this one source compiled several times (MC_TU = 0: C ABI + host helpers;
// 1..5: the engine + kernels of one group of specs each), so the per-spec kernels compile in parallel.
#ifndef MC_TU
#define MC_TU -1  // single translation unit: everything
#endif
}  // namespace mc
#include "engine_kernels.h"   // namespace mc { ... every kernel ... }
#include "engine_pairs.h"     // k_expand_pairs: the by-pairs expand + insert + write kernel (specs with S::PAIR_FAMILIES)
#include "engine_sim.h"       // k_simulate: simulation mode, one lane per random walk (mc_engine_simulate)
#include "engine_behaviours.h"  // k_behaviours: recorded behaviours against the model, one wavefront per behaviour (mc_engine_behaviours)
#include "engine_coverage.h"  // k_coverage_generated / k_coverage_distinct: per-action counts (MC_F_COVERAGE, mc_engine_coverage)
#include "engine_violations.h"  // k_viol_stored / k_viol_frontier: what a flagged level holds (MC_F_CONTINUE, mc_engine_violations)
#include "engine_graph.h"     // k_graph_index / k_graph_degree / k_graph_fill / k_live_proc: the state graph in CSR form (mc_engine_graph)
#include "state_graph.h"      // StateGraph: what consumes that form (reads, mc_engine_scc, mc_engine_liveness), and the device scans; compiled once
namespace mc {

// ------------------------------------------------------------------------------------- host side
struct EngineBase {
    DevBuf<int32_t> owned_device_blob;  // program image of a compiled PlusCal spec (spec_vm.h)
    uint64_t program_hash = 0;          // ... and a hash of that image + its entry points: what a checkpoint of it is matched by
    mc_progress_fn progress_fn = nullptr;  // mc_engine_set_progress
    void *progress_user = nullptr;
    double progress_interval = 1.0;
    std::chrono::steady_clock::time_point progress_last;
    bool stop_requested = false;  // mc_engine_request_stop (from a progress callback): run() stops before the next level, verdict "budget"
    void report_progress(uint32_t levels, uint64_t generated, uint64_t distinct, uint64_t queue) {
        if (!progress_fn) return;
        const auto now = std::chrono::steady_clock::now();
        if (std::chrono::duration<double>(now - progress_last).count() < progress_interval) return;
        progress_last = now;
        progress_fn(progress_user, levels, generated, distinct, queue);
    }
    virtual ~EngineBase() = default;
    virtual int run(mc_result *out) = 0;
    virtual int step(uint32_t levels, mc_result *out) = 0;
    virtual int trace(uint8_t *states_out, int32_t *actions_out, size_t *n_inout) = 0;
    virtual int kernel_stats(mc_kernel_stats *out) = 0;
    virtual int read_states(uint64_t first, uint64_t count, uint8_t *out) = 0;
    virtual int debug_reexpand(unsigned extra_flags, double *ms) = 0;
    virtual int debug_phases(uint64_t *out48, int reset) = 0;
    virtual int debug_flags(uint32_t set, uint32_t clear) = 0;
    virtual int seen_layout(uint64_t *buckets, uint32_t *slots) = 0;
    virtual int checkpoint(const char *path) = 0;
    virtual int restore(const char *path) = 0;
    virtual int shard_begin() = 0;
    virtual int shard_begin_replicated(uint64_t min_frontier, uint64_t max_distinct, uint64_t max_levels, uint64_t *levels_out, uint32_t *nlevels) = 0;
    virtual int shard_level_size(uint64_t *n) = 0;
    virtual int shard_set_stream(void *hip_stream, int enable) = 0;
    virtual int shard_expand_launch(unsigned slot, uint64_t first, uint64_t count, uint64_t send_cap) = 0;
    virtual int shard_expand_finish(unsigned slot, uint64_t *send_fp, uint64_t send_cap, uint64_t *send_counts) = 0;
    virtual int shard_probe(const uint64_t *recv_fp, uint64_t n, uint8_t *answers) = 0;
    virtual int shard_expand_pack(unsigned slot, uint64_t *send_fp, uint64_t cap) = 0;
    virtual int shard_probe_pack(const uint64_t *recv_fp, uint64_t cap, uint8_t *answers) = 0;
    virtual int shard_keep_pack(unsigned slot, const uint8_t *answers_back, uint64_t cap) = 0;
    virtual int shard_wait_keep(unsigned slot) = 0;
    virtual int shard_materialise(unsigned slot, const uint8_t *answers_back, uint8_t *send_states, uint64_t send_cap, uint64_t *send_counts) = 0;
    virtual int shard_ingest(const uint8_t *recv_states, uint64_t n) = 0;
    virtual int shard_keep(unsigned slot, const uint8_t *answers_back, uint64_t *n_new) = 0;
    virtual int shard_end_level(uint64_t *new_local) = 0;
    virtual int shard_counters(uint64_t *generated, uint64_t *distinct_local, int32_t *verdict) = 0;
    virtual int shard_check_frontier() = 0;
    virtual int shard_materialise_parents(unsigned slot, uint64_t *send_parents) = 0;
    virtual int shard_ingest_parents(const uint64_t *recv_parents, uint64_t n, unsigned src_rank) = 0;
    virtual int shard_violation(int32_t *found, uint64_t *idx, uint32_t *slot, int32_t *verdict, int32_t *invariant) = 0;
    virtual int shard_fetch(uint64_t idx, uint8_t *state_out, uint32_t *parent_rank, uint64_t *parent_idx, uint32_t *parent_slot) = 0;
    virtual int shard_info(void **main_stream, uint64_t *chunk_states, int32_t *traced) = 0;
    virtual int shard_note_levels(const uint64_t *levels, uint32_t n, int32_t verdict) = 0;
    virtual int shard_resume(uint64_t *levels_out, uint32_t *nlevels) = 0;
    virtual int shard_checkpoint(const char *path) = 0;
    virtual int shard_restore(const char *path) = 0;
    virtual size_t state_bytes() const = 0;
    virtual int narrow_rows() const = 0;
    mc_config created_with;   // make_engine: what mc_engine_create was given (an engine is made again from it: shard_side)
    virtual int simulate(const mc_sim_opts *opts, mc_sim_result *out) = 0;
    virtual int behaviours(const mc_beh_opts *opts, mc_beh_verdict *out, mc_beh_result *result) = 0;
    virtual int behaviours_refused() = 0;   // MC_OK, or why this engine checks no behaviours (mc_last_error says it)
    virtual const mc_spec_desc *spec_desc() const = 0;
    virtual int coverage(mc_action_coverage *out, size_t *n_inout) = 0;
    virtual int violations(mc_violations_info *info, mc_violation *out, size_t *n_inout) = 0;
    virtual int violation_trace(size_t k, uint8_t *states_out, int32_t *actions_out, size_t *n_inout) = 0;
    // ---- the state graph (state_graph.h).  The two calls that walk the arena with the lowering's kernels are the engine's; the rest
    // consumes the CSR arrays and is the StateGraph's.  Engine<S>::alloc says where the graph's engine keeps what those calls need.
    StateGraph gr;
    bool sharded = false;                               // shard_count > 1: no graph
    hipStream_t graph_stream = nullptr;                 // the engine's main stream
    const std::vector<uint64_t> *graph_levels = nullptr;   // the level table of the last search
    virtual int graph(mc_graph_info *out) = 0;
    virtual int predicates(uint64_t first, uint64_t count, uint32_t *bits_out) = 0;
    // every liveness check (live_query.h): prop for a property's name and refusal; of the outputs, those the C entry has
    virtual int liveness_run(const LiveQuery &q, const mc_live_property *prop, mc_live_info *out, mc_live_check_info *check_out, mc_live_strong_info *strong_out) = 0;
    int liveness_edge_units(uint64_t first, uint64_t count, int8_t *unit_out) { return gr.live_unit_read(first, count, unit_out); }
    int graph_read(uint64_t first, uint64_t count, uint64_t *offsets_out, uint32_t *dst_out, int32_t *action_out, size_t *nedges_inout) {
        return gr.read(first, count, offsets_out, dst_out, action_out, nedges_inout);
    }
    int scc(mc_scc_info *out) {
        memset(out, 0, sizeof *out);
        if (sharded) { set_error("mc_engine_scc: not available for a sharded engine (shard_count > 1)"); return MC_EBADCFG; }
        if (!gr.built) { mc_graph_info gi; if (int rc = graph(&gi)) return rc; }
        return gr.scc(graph_stream, out);
    }
    int scc_read(uint64_t first, uint64_t count, uint32_t *scc_out) { return gr.scc_read(first, count, scc_out); }
    int liveness_components(uint64_t first, uint64_t count, uint32_t *scc_out) { return gr.live_scc_read(first, count, scc_out); }
    int liveness_trace(uint32_t *prefix_out, size_t *nprefix_inout, uint32_t *cycle_out, size_t *ncycle_inout) {
        return gr.live_trace(*graph_levels, prefix_out, nprefix_inout, cycle_out, ncycle_inout);
    }
};

static uint64_t round_pow2(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

struct KTimer {
    std::vector<Event> pool;
    struct Pending { int which; size_t e0, e1; uint64_t units; };
    std::vector<Pending> pending;
    size_t used = 0;
    bool enabled = false;
    hipEvent_t get() {
        if (used == pool.size()) pool.emplace_back(hipEventDefault);
        return pool[used++].get();
    }
    void resolve(mc_kernel_stat *stats /*[3]*/) {
        for (auto &p : pending) {
            float ms = 0;
            hipEventElapsedTime(&ms, pool[p.e0].get(), pool[p.e1].get());
            stats[p.which].launches++;
            stats[p.which].ms_total += ms;
            stats[p.which].units += p.units;
        }
        pending.clear();
        used = 0;
    }
};

// specs whose stored row is not the row the C ABI hands out (spec_gen.h: generated code packs its cells): S::EXPORT_WORDS, S::export_row
template <class S, class = void>
struct HasExport : std::false_type {};
template <class S>
struct HasExport<S, decltype((void)S::EXPORT_WORDS)> : std::true_type {};
// ... with a public width that depends on the model's constants, and rows that come IN through S::import_row (spec_raft_packed.h)
template <class S, class = void>
struct RaftPacked : std::false_type {};
template <class S>
struct RaftPacked<S, decltype((void)S::RAFT_PACKED)> : std::true_type {};
template <class S>
static size_t export_words_of(const typename S::Params &prm, int W) {
    if constexpr (RaftPacked<S>::value) return (size_t)S::export_words(prm);
    else if constexpr (HasExport<S>::value) return (size_t)S::EXPORT_WORDS;
    else return (size_t)W;
}
template <class S, class = void>
struct PackedRows : std::false_type {};
template <class S>
struct PackedRows<S, decltype((void)S::PACKED_ROWS)> : std::integral_constant<bool, S::PACKED_ROWS> {};

// what a violation key (engine_kernels.h viol_key; the same kinds in a simulation's: sim_walk.h) says
static_assert((unsigned)SIM_VK_INVARIANT == VK_INVARIANT && (unsigned)SIM_VK_ASSERT == VK_ASSERT && (unsigned)SIM_VK_DEADLOCK == VK_DEADLOCK, "one verdict_of_kind");
static int32_t verdict_of_kind(unsigned kind) {
    return kind == VK_INVARIANT ? MC_V_INVARIANT : kind == VK_ASSERT ? MC_V_ASSERT : kind == VK_DEADLOCK ? MC_V_DEADLOCK : MC_V_SPECERR;
}
struct Viol {
    unsigned kind, slot;
    int32_t verdict, invariant;  // invariant: its index, or -1
    explicit Viol(unsigned long long key)
        : kind((unsigned)(key & 7u)), slot((unsigned)(key >> 8 & 0xffffu)), verdict(verdict_of_kind(kind)), invariant(kind == VK_INVARIANT ? (int32_t)(key >> 3 & 31u) : -1) {}
    bool extra_state() const { return kind == VK_INVARIANT && slot < SLOT_PARENT; }  // the violating successor itself ends the trace
};

// ------------------------------------------------------------------------------- checkpoint files
// Two formats, one identity prefix: a fused engine's file (mc_engine_checkpoint) and a rank's file of a sharded run (mc_shard_checkpoint).
// Both are: header, level table (nlevels words), [the rank's counters], then device sections as they lie in HBM (Engine::ck_sections).
struct CkIdent {
    char magic[8];
    uint32_t spec_id, nparams;
    int64_t params[16];  // of a compiled program: params[0] = the hash of its image (its parameter is a host pointer)
    uint32_t words, has_trace;
};
struct CkHeader {
    CkIdent id;
    uint64_t distinct, generated, cells, lo, hi, nlevels;
};
struct ShCkHeader {
    CkIdent id;
    uint32_t rank, world;
    uint64_t table_cap, lo, hi, next, dup, nlevels;
};
// the counters a per-rank checkpoint carries, field by field (the file held a raw DevCounters, whose layout —
// padding, alignment, members — changes with the kernels; "TLAMCSK1" files are refused as "not a per-rank checkpoint file")
struct ShCkCounters {
    uint64_t arena_next, viol_key, via_list;
    uint64_t generated[NSHARD], cells[NSHARD];
    uint32_t error, pad;
};
// the files' layout is fixed (files written by earlier builds restore; tests edit bytes at these offsets)
static_assert(sizeof(CkIdent) == 152 && offsetof(CkIdent, spec_id) == 8 && offsetof(CkIdent, params) == 16 && offsetof(CkIdent, words) == 144 && offsetof(CkIdent, has_trace) == 148, "checkpoint identity");
static_assert(sizeof(CkHeader) == 200 && offsetof(CkHeader, distinct) == 152 && offsetof(CkHeader, generated) == 160 && offsetof(CkHeader, cells) == 168 &&
              offsetof(CkHeader, lo) == 176 && offsetof(CkHeader, hi) == 184 && offsetof(CkHeader, nlevels) == 192, "TLAMCCK1 header");
static_assert(sizeof(ShCkHeader) == 208 && offsetof(ShCkHeader, rank) == 152 && offsetof(ShCkHeader, world) == 156 && offsetof(ShCkHeader, table_cap) == 160 &&
              offsetof(ShCkHeader, lo) == 168 && offsetof(ShCkHeader, hi) == 176 && offsetof(ShCkHeader, next) == 184 && offsetof(ShCkHeader, dup) == 192 &&
              offsetof(ShCkHeader, nlevels) == 200, "TLAMCSK2 header");
static_assert(NSHARD == 8 && sizeof(ShCkCounters) == 160 && offsetof(ShCkCounters, generated) == 24 && offsetof(ShCkCounters, cells) == 88 && offsetof(ShCkCounters, error) == 152, "TLAMCSK2 counters");
// what tells the two formats apart: the magic, and the words of the messages (`who` + ": " + ...)
struct CkFormat { const char *magic, *writer, *reader, *not_ours, *other_program; };
static constexpr CkFormat CK_FUSED{"TLAMCCK1", "checkpoint", "restore", "not a checkpoint file",
                                   "the checkpoint was written by another compiled program (algorithm, constants, invariants or constraints differ)"};
static constexpr CkFormat CK_RANK{"TLAMCSK2", "mc_shard_checkpoint", "mc_shard_restore", "not a per-rank checkpoint file (of this library version)",
                                  "the checkpoint was written by another compiled program"};
struct CkPart { void *p; size_t bytes; };  // a run of bytes of a checkpoint file, in host or in device memory
struct FileCloser { FILE *f; ~FileCloser() { if (f) fclose(f); } };

template <class S>
struct Engine : EngineBase {
    using Params = typename S::Params;
    int W = 1;  // 64-bit words per packed state
    unsigned max_slots = 1;
    Params prm;
    mc_spec_desc desc;
    mc_config cfg;
    // ---- HIP resources: streams first (members go in reverse order: the streams outlive every event and buffer)
    Stream stream, stream2;  // expand+insert on `stream`, materialise on `stream2`
    // The chunks of ONE level are independent of each other (they read the frontier, probe / insert with atomics, take arena indices
    // with atomics): the odd ones go to a stream of their own, so that the first workgroups of chunk c+1 fill the CUs the last
    // workgroups of chunk c leave idle (a launch of 2^23 parents is 32 rounds of the 2048 resident workgroups: the last one is half
    // empty) instead of waiting for the stream order.  $TLAMC_EXPAND_STREAMS = 2 switches it on (A/B; off by default until measured).
    Stream stream_b;
    Event ev_level, ev_e[2], ev_m[2];
    DevBuf<uint64_t> d_arena, d_table, d_cand, d_inittmp;
    DevBuf<uint32_t> d_newlist, d_parent;
    DevBuf<uint64_t> d_newfp;  // fingerprints of the new-list entries (specs with apply_known_fp)
    DevBuf<uint16_t> d_nsl, d_pslot;
    DevBuf<uint8_t> d_prank;  // sharded runs with MC_F_TRACE: rank a state's parent lives on (0xff = this rank)
    DevBuf<DevCounters> d_ctr;
    PinnedBuf<DevCounters> h_ctr;
    DevBuf<LevelCtl> d_lc;
    PinnedBuf<LevelCtl> h_lc;
    uint64_t table_cap = 0, arena_cap = 0, chunk = 0, row_stride = 0, seg_cap = 0;
    bool seen_sparse = false, use_matrix = false;
    bool no_slices = getenv("TLAMC_NOSLICE") != nullptr;
    // fused runs of a by-family spec: the expand wavefronts write their own survivors (MC_F_NOINWAVE = A/B: everything through the
    // new-list and k_materialise, as in rounds 1-3)
    double inwave_growth_limit = getenv("TLAMC_INWAVE_GROWTH") ? atof(getenv("TLAMC_INWAVE_GROWTH")) : 10.0;  // (A/B knob.  Round 4, profiles/r04l:
    // t3 — levels grow by at most 2.2 x — was best with every level in-wave, the 5-server model — 2.4 x and more on all 18 levels — with
    // none, 230.6 against 239.0 ms: the limit was 2.3.  Round 5: with the writer's scratch traffic gone the in-wave tail wins there too,
    // 191.9 / 192.1 against 205.0 / 203.0 ms at 2.3 (profiles/r05i_raft5_inwave_growth.jsonl); 10 = in effect every level)
    KTimer timer;
    mc_kernel_stat kstat[3];
    // ---- the fused run (run / step) and what it left behind: counters, level table, counterexample
    struct Fused {
        bool have_run = false, have_viol = false;
        unsigned long long last_viol = ~0ull;
        std::vector<uint64_t> level_start;
        uint64_t last_distinct = 0, last_generated = 0, cells = 0, inwave = 0;  // cells, inwave: for mc_kernel_stats
        uint64_t stop_frontier = 0, lo = 0, hi = 0;  // run() stops before a level of >= stop_frontier states (0 = never); the frontier it stopped with
        bool mat_inwave_level = false;     // the level being enqueued writes in-wave: k_materialise sees the overflow only
        uint64_t mat_list_hint = 0;        // states per chunk the level before sent through the new-list
    } fr;
    // ---- hand-over to the next run(): from restore() (a checkpoint file) or step() (in place: the stopped run's seen-set is still valid)
    struct HandOver {
        bool pending = false, in_place = false;
        uint64_t distinct = 0, generated = 0, cells = 0, lo = 0;
        std::vector<uint64_t> level_start;
    } ck;
    // ---- the sharded step API (mc_shard_*)
    // Two expand slots: the route-mode expand of chunk r+1 (on `stream`) overlaps the exchange, probe and keep /
    // materialise of chunk r (kernels on `stream2`, collectives on the caller's stream).
    struct ShSlot {
        DevBuf<uint64_t> rt_fp;
        DevBuf<uint32_t> rt_src, pend_src;  // pend_src.n = the slot's pending-list capacity (shard_alloc)
        DevBuf<PaddedCounter> rt_cur;  // [nranks*NSHARD] route cursors
        uint64_t rt_subcap = 0, pend_total = 0, chunk_base = 0, count = 0, ncols = 0;
        BlockPlan plan;          // of the slot's last shard_materialise (for shard_materialise_parents)
        uint64_t moved = 0;
        OwnerOffsets pend_off;
        bool launched = false, keep_pending = false;
    };
    struct Shard {
        uint64_t lo = 0, hi = 0, next = 0;  // local frontier [lo, hi), arena fill level
        uint64_t dup = 0;                   // states of the replicated prefix that other ranks count (shard_begin_replicated)
        ShSlot sl[2];
        DevBuf<uint32_t> d_new_src, d_incl;
        DevBuf<unsigned long long> d_ends;
        PinnedBuf<unsigned long long> h_ends;
        PinnedBuf<PaddedCounter> h_cur;  // pinned copy of one slot's route cursors
        DevBuf<char> d_scan_tmp;
        // Side stream of the sharded path.  By default the engine's own second stream, and every step call returns
        // with its work finished.  A caller that runs its collectives on a HIP stream hands that stream over with
        // shard_set_stream: compaction / probe / keep / materialise / ingest are then enqueued on it WITHOUT host
        // synchronisation (stream order ties them to the caller's all-to-alls), and only the calls that must return
        // counts to the host wait.
        hipStream_t ext_stream = nullptr;
        bool ext_side = false;
        Event ev_slot[2], ev_keep[2], ev_ans;
        // Three kinds of kernels append states at arena_next (the chunk's locally owned new states, keep, ingest) and they run on
        // different streams: one event chains them, each appender waits for the previous one and records when it is enqueued.
        Event ev_append;
        // fixed-capacity rounds (nothing of a round waits for the host; sizes travel in band; errors surface at shard_end_level)
        Event ev_exp[2];
        // the slot's new-list segment and its counters (parity = slot) are read by the local materialise + commit on the second
        // stream: the NEXT expand into the same slot waits for them (a host that never blocks enqueues expands back to back)
        Event ev_mat[2];
        std::vector<uint64_t> levels;  // the whole job's level table (shard_note_levels): what a per-rank checkpoint carries
        bool ck_ok = false, resume = false;
        std::unique_ptr<mc_result> prefix_res{new mc_result()};  // of the replicated prefix: large (level table), so not on the stack
    } sh;
    // ---- simulation (mc_engine_simulate): the walk buffers, allocated on first use, and the counterexample of the last simulation
    struct Sim {
        DevBuf<uint64_t> buf[2];
        DevBuf<uint32_t> wst;
        DevBuf<SimCounters> ctr;
        std::vector<uint64_t> trace_rows;  // rows in S's layout
        std::vector<int32_t> trace_acts;   // ... and their action ids
        size_t trace_n = 0;
    } sim;
    // ---- behaviour checking (mc_engine_behaviours): a round's candidate sets, observations and verdicts, allocated on first use
    struct Beh {
        DevBuf<uint64_t> set[2], stage, rows, first, carry, mask;
        DevBuf<mc_beh_verdict> out;
        DevBuf<BehCounters> ctr;
    } beh;
    // ---- coverage (MC_F_COVERAGE, mc_engine_coverage): per-action histograms, bin 0 = Init, bin a + 1 = action id a
    struct Cov {
        bool on = false;
        int nbins = 0;
        DevBuf<unsigned long long> bins;   // [2 * nbins]: generated, then distinct; bumped by the kernels of engine_coverage.h
        std::vector<uint64_t> host;        // the bins as the last run left them (+ Init's generated, which no kernel counts)
        uint64_t init_generated = 0;
    } cov;
    // ---- -continue (MC_F_CONTINUE, mc_engine_violations): what the flagged levels of the last search held
    struct Vio {
        bool on = false;
        DevBuf<ViolBins> bins;             // bumped by the kernels of engine_violations.h
        ViolBins host;                     // ... as the last flagged level left them
        bool have_first = false, fatal = false;
        unsigned long long first_key = ~0ull;   // DevCounters::viol_key of the first flagged level: what the run reports
        uint32_t flagged_levels = 0, passes = 0;
    } vio;

    // slot slices of a generic-kernel launch (k_expand_insert): as many as it takes to give the device a few thousand wavefronts,
    // for specs whose slots all go through the loop (no unrolled prefix) and that have enough of them; TLAMC_NOSLICE=1 = A/B
    unsigned slices_for(uint64_t ncols, bool blind) const {
        // (a lowering asks for it with SLICE_SLOTS: worth it when one slot evaluation is expensive — the Paxos family's witness
        // enumeration, the bytecode interpreter; for atomic_add's two-instruction slots the slices only repeat the parent loads)
        if (!WantsSlices<S>::value || S::FIX_SLOTS != 0 || UsesFamilies<S>::value || pairs_only() || use_matrix || max_slots < 16 || no_slices) return 1;  // (the by-pairs kernel has no slices: its lanes are pairs already)
        const uint64_t waves = (ncols + 63) / 64;
        uint64_t sg = blind ? 32 : (16384 + waves - 1) / waves;  // a blind level launches its CAPACITY: the frontier itself is smaller
        if (sg > 32) sg = 32;
        if (sg > max_slots / 4) sg = max_slots / 4;
        return sg < 1 ? 1u : (unsigned)sg;
    }
    uint64_t seen_arg() const { return seen_sparse ? ((table_cap / MC_SPARSE_SLOTS) | SEEN_SPARSE) : table_cap / 8; }
    unsigned nranks() const { return cfg.shard_count > 1 ? cfg.shard_count : 1; }

    int alloc() {
        W = S::words(prm);
        max_slots = (unsigned)S::max_slots(prm);
        use_matrix = (cfg.flags & MC_F_MATRIX) != 0;
        HIP_TRY(hipSetDevice(cfg.device));
        HIP_TRY(stream.create());
        sharded = cfg.shard_count > 1;
        graph_stream = stream;
        graph_levels = &fr.level_start;
        {   // A/B knob (measured in DESIGN.md section 4): TLAMC_PRIO=1 gives the materialise stream the highest priority, =2 the lowest
            const char *pe = getenv("TLAMC_PRIO");
            int lo_p = 0, hi_p = 0;
            hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);  // lo_p = least, hi_p = greatest priority (numerically smaller)
            if (pe && *pe == '1') HIP_TRY(stream2.create(hi_p));
            else if (pe && *pe == '2') HIP_TRY(stream2.create(lo_p));
            else HIP_TRY(stream2.create());
        }
        for (int i = 0; i < 2; i++) { HIP_TRY(ev_e[i].create()); HIP_TRY(ev_m[i].create()); }
        {
            const char *es = getenv("TLAMC_EXPAND_STREAMS");
            if (es && *es == '2') {
                HIP_TRY(stream_b.create());
                HIP_TRY(ev_level.create());
            }
        }
        table_cap = cfg.table_capacity ? cfg.table_capacity : (1ull << 24);
        table_cap = (table_cap + 63) / 64 * 64;  // whole 8-slot buckets; any size (seen_insert), at most 2^32 buckets
        if (table_cap / 8 > 0xffffffffull) { set_error("table_capacity: at most 2^35 - 8 slots per device"); return MC_EBADCFG; }
        arena_cap = cfg.arena_capacity ? cfg.arena_capacity : (1ull << 22);
        arena_cap = (arena_cap + 63) & ~63ull;
        if (arena_cap >= (1ull << 32) - 1) { set_error("arena_capacity must be < 2^32 states"); return MC_EBADCFG; }
        // a table that can never be more than a third full is probed 32 bytes at a time (seen_insert); $TLAMC_SPARSE_RATIO = A/B knob
        // for "a third" (slots per arena state, default 3)
        static const double sparse_ratio = getenv("TLAMC_SPARSE_RATIO") && atof(getenv("TLAMC_SPARSE_RATIO")) >= 1.25 ? atof(getenv("TLAMC_SPARSE_RATIO")) : 3.0;
        seen_sparse = (double)table_cap >= sparse_ratio * (double)arena_cap && table_cap / MC_SPARSE_SLOTS <= 0xffffffffull && !getenv("TLAMC_DENSE_TABLE");
        chunk = cfg.chunk_states ? cfg.chunk_states : (1ull << 18);
        chunk = (chunk + 255) & ~255ull;
        if (chunk > (1ull << 24) - 256) chunk = (1ull << 24) - 256;  // a column index must fit 24 bits (new-list entries: (slot << 24) | column)
        if (max_slots > 255) { set_error("spec has more than 255 action slots per state"); return MC_EBADCFG; }
        row_stride = chunk + 256;
        HIP_TRY(d_arena.alloc(arena_cap * W));
        HIP_TRY(d_table.alloc(table_cap));
        HIP_TRY(d_cand.alloc((size_t)(use_matrix ? max_slots : 1) * row_stride));
        seg_cap = (row_stride / NSHARD + 256) * max_slots;
        seg_cap += seg_cap / 64 + 65;   // (round 6: an in-wave writer parks its overflow here as chunks of 64 entries + a link: 65 / 64 of the worst case)
        HIP_TRY(d_newlist.alloc((size_t)2 * NSHARD * seg_cap));
        if (HasKnownFp<S>::value && !use_matrix) HIP_TRY(d_newfp.alloc((size_t)2 * NSHARD * seg_cap));
        {
            const uint64_t ni = S::num_init(prm);
            HIP_TRY(d_inittmp.alloc((size_t)(ni < chunk ? ni : chunk) * W));
        }
        HIP_TRY(d_nsl.alloc(row_stride));
        if (cfg.flags & MC_F_TRACE) {
            HIP_TRY(d_parent.alloc(arena_cap));
            HIP_TRY(d_pslot.alloc(arena_cap));
            if (cfg.shard_count > 1) {
                HIP_TRY(d_prank.alloc(arena_cap));
                HIP_TRY(hipMemset(d_prank, 0xff, arena_cap));
            }
        }
        HIP_TRY(d_ctr.alloc(1));
        HIP_TRY(h_ctr.alloc(1));
        HIP_TRY(d_lc.alloc(1));
        HIP_TRY(h_lc.alloc(1));
        timer.enabled = (cfg.flags & MC_F_TIMING) != 0;
        if (cfg.flags & MC_F_COVERAGE) {
            cov.nbins = CovAction<S>::nbins(prm);
            if (cov.nbins > COV_MAX_BINS) { set_error("MC_F_COVERAGE: the model has more actions than the coverage histogram has bins (" + std::to_string(COV_MAX_BINS - 1) + ")"); return MC_EBADCFG; }
            HIP_TRY(cov.bins.alloc((size_t)2 * cov.nbins));
            HIP_TRY(hipMemset(cov.bins, 0, (size_t)2 * cov.nbins * sizeof(unsigned long long)));
            cov.host.assign((size_t)2 * cov.nbins, 0);
            cov.on = true;
        }
        if (cfg.flags & MC_F_CONTINUE) {
            if (ViolModel<S>::ninv(prm) > VIOL_MAX_INV) { set_error("MC_F_CONTINUE: the model has more than 32 invariants"); return MC_EBADCFG; }
            HIP_TRY(vio.bins.alloc(1));
            vio.on = true;
        }
        return MC_OK;
    }

    // ------------------------------------------------------------------------------- -continue (engine_violations.h)
    // All on `stream`, behind the kernels of the level they look at, and only for a level that set the violation key.
    int viol_begin() {
        memset(&vio.host, 0, sizeof vio.host);
        for (int i = 0; i < VIOL_CELLS; i++) vio.host.first[i] = ~0ull;
        vio.have_first = vio.fatal = false;
        vio.first_key = ~0ull;
        vio.flagged_levels = vio.passes = 0;
        HIP_TRY(hipMemcpyAsync(vio.bins, &vio.host, sizeof vio.host, hipMemcpyHostToDevice, stream));
        return MC_OK;
    }
    void viol_stored(uint64_t lo, uint64_t hi) {
        for (uint64_t c0 = lo; c0 < hi; c0 += chunk) {
            const uint64_t c1 = c0 + chunk < hi ? c0 + chunk : hi;
            hipLaunchKernelGGL(k_viol_stored<S>, dim3((unsigned)((c1 - c0 + 255) / 256)), dim3(256), 0, stream, prm, (const uint64_t *)d_arena,
                               (const uint32_t *)d_parent, (const uint16_t *)d_pslot, c0, c1, vio.bins.p);
            vio.passes++;
        }
    }
    void viol_frontier(uint64_t lo, uint64_t hi) {
        each_chunk(lo, hi, [&](uint64_t c0, uint64_t c1, uint64_t ncols) {
            hipLaunchKernelGGL(k_viol_frontier<S>, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, stream, prm, (const uint64_t *)d_arena,
                               c0, c1, ncols, (unsigned)cfg.flags, vio.bins.p);
            vio.passes++;
        });
    }
    // The level that expanded [lo, hi) and stored [hi, new_hi) has set the key (h_ctr is the host's copy of the counters after it):
    // remember the first key, run the passes, and either leave the key (a fatal kind: the level loop ends on it) or clear it on the
    // device, stream-ordered, and in the host's copy.  expanded = false: only stored states were looked at (Init; check_frontier).
    int viol_level(uint64_t lo, uint64_t hi, uint64_t new_hi, bool expanded) {
        if (!vio.have_first) { vio.have_first = true; vio.first_key = h_ctr->viol_key; }
        vio.flagged_levels++;
        if (expanded) viol_frontier(lo, hi);
        if (!expanded || ChecksOnExpand<S>::value) viol_stored(lo, hi);
        else viol_stored(hi, new_hi);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&vio.host, vio.bins, sizeof vio.host, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (vio.host.count[VIOL_BINS + VIOL_BIN_FATAL]) { vio.fatal = true; return MC_OK; }
        hipLaunchKernelGGL(k_clear_viol_key, dim3(1), dim3(1), 0, stream, d_ctr.p);
        h_ctr->viol_key = ~0ull;
        return MC_OK;
    }
    uint32_t level_of(uint64_t idx) const {   // 1-based BFS level of an arena index
        const auto it = std::upper_bound(fr.level_start.begin(), fr.level_start.end(), idx);
        return (uint32_t)(it - fr.level_start.begin());
    }
    // entry k of mc_engine_violations: what it is and where its evidence lies.  shown: 0 nothing, 1 a stored state, 2 a (state, slot) key
    struct ViolEntry { mc_violation v; int shown; unsigned long long key; };
    size_t viol_entries() const { return (size_t)ViolModel<S>::ninv(prm) + ((cfg.flags & MC_F_DEADLOCK) ? 1 : 0) + (vio.fatal ? 1 : 0); }
    int viol_entry(size_t k, ViolEntry &e) {
        const size_t ninv = (size_t)ViolModel<S>::ninv(prm);
        memset(&e, 0, sizeof e);
        e.v.invariant = -1;
        e.v.first_state = ~0ull;
        const bool dl = (cfg.flags & MC_F_DEADLOCK) != 0;
        int bin;
        if (k < ninv) { bin = (int)k; e.v.kind = MC_V_INVARIANT; e.v.invariant = (int32_t)k; }
        else if (dl && k == ninv) { bin = VIOL_BIN_DEADLOCK; e.v.kind = MC_V_DEADLOCK; }
        else if (vio.fatal && k == ninv + (dl ? 1 : 0)) bin = VIOL_BIN_FATAL;
        else { set_error("mc_engine_violations: entry out of range"); return MC_EBADCFG; }
        e.v.states = vio.host.count[bin];
        e.v.outside = vio.host.count[VIOL_BINS + bin];
        if (e.v.states) { e.shown = 1; e.v.first_state = vio.host.first[bin]; }
        else if (e.v.outside) {
            e.shown = 2;
            e.key = vio.host.first[VIOL_BINS + bin];
            e.v.first_state = viol_idx(e.key);
            if (bin == VIOL_BIN_FATAL) { const Viol f(e.key); e.v.kind = f.verdict; e.v.invariant = f.invariant; }
        }
        if (e.shown) {   // (a stored state's shortest behaviour has as many states as its level: nothing is read from the device here)
            e.v.first_level = level_of(e.v.first_state);
            e.v.trace_len = e.v.first_level + (e.shown == 2 && Viol(e.key).extra_state() ? 1u : 0u);
        }
        return MC_OK;
    }
    int violations(mc_violations_info *info, mc_violation *out, size_t *n_inout) override {
        if (!vio.on) { set_error("mc_engine_violations: the engine was created without MC_F_CONTINUE"); return MC_ESTATE; }
        if (!fr.have_run) { set_error("mc_engine_violations: needs a search of this engine that returned a result"); return MC_ESTATE; }
        const size_t n = viol_entries();
        if (info) { info->flagged_levels = vio.flagged_levels; info->passes = vio.passes; info->fatal = vio.fatal ? 1u : 0u; info->pad = 0; }
        if (n > *n_inout || !out) { *n_inout = n; set_error("mc_engine_violations: buffer too small"); return MC_EBADCFG; }
        HIP_TRY(hipSetDevice(cfg.device));
        for (size_t k = 0; k < n; k++) {
            ViolEntry e;
            if (int rc = viol_entry(k, e)) return rc;
            out[k] = e.v;
        }
        *n_inout = n;
        return MC_OK;
    }
    int violation_trace(size_t k, uint8_t *states_out, int32_t *actions_out, size_t *n_inout) override {
        if (!vio.on) { set_error("mc_engine_violation_trace: the engine was created without MC_F_CONTINUE"); return MC_ESTATE; }
        if (!fr.have_run) { set_error("mc_engine_violation_trace: needs a search of this engine that returned a result"); return MC_ESTATE; }
        if (k >= viol_entries()) { set_error("mc_engine_violation_trace: entry out of range"); return MC_EBADCFG; }
        HIP_TRY(hipSetDevice(cfg.device));
        ViolEntry e;
        if (int rc = viol_entry(k, e)) return rc;
        if (!e.shown) { set_error("mc_engine_violation_trace: the entry has nothing to show"); return MC_EBADCFG; }
        const bool extra = e.shown == 2 && Viol(e.key).extra_state();
        return chain_trace(e.v.first_state, extra, extra ? Viol(e.key).slot : 0u, states_out, actions_out, n_inout);
    }

    // ------------------------------------------------------------------------------- coverage (engine_coverage.h)
    // All on `stream`, behind the expand kernels of the level they count: the arena rows and trace records they read are final by then.
    // The states [lo, hi) in the chunks the expand kernel saw (engine_coverage.h: each_chunk), at this engine's chunk size
    template <class F>
    void each_chunk(uint64_t lo, uint64_t hi, F &&f) { mc::each_chunk(lo, hi, chunk, f); }
    // generated: the states [lo, hi) a level expanded
    void cov_generated(uint64_t lo, uint64_t hi) {
        each_chunk(lo, hi, [&](uint64_t c0, uint64_t c1, uint64_t ncols) {
            hipLaunchKernelGGL(k_coverage_generated<S>, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, stream, prm, (const uint64_t *)d_arena,
                               c0, c1, ncols, cov.bins.p, cov.nbins);
        });
    }
    // distinct: the states [lo, hi) a level added (or Init stored), by their trace records
    void cov_distinct(uint64_t lo, uint64_t hi) {
        for (uint64_t c0 = lo; c0 < hi; c0 += chunk) {
            const uint64_t c1 = c0 + chunk < hi ? c0 + chunk : hi;
            hipLaunchKernelGGL(k_coverage_distinct<S>, dim3((unsigned)((c1 - c0 + 255) / 256)), dim3(256), 0, stream, prm, (const uint64_t *)d_arena,
                               (const uint32_t *)d_parent, (const uint16_t *)d_pslot, c0, c1, cov.bins.p + cov.nbins, cov.nbins);
        }
    }
    // a search that starts over: empty bins, then what is in the arena already — Init's states, or (a restored checkpoint, whose parent
    // pointers came with it) every level the checkpointed run expanded, [0, expanded), and every state it stored, [0, stored)
    int cov_begin(uint64_t expanded, uint64_t stored) {
        HIP_TRY(hipMemsetAsync(cov.bins, 0, (size_t)2 * cov.nbins * sizeof(unsigned long long), stream));
        cov.init_generated = S::num_init(prm);
        cov_generated(0, expanded);
        cov_distinct(0, stored);
        return MC_OK;
    }
    int cov_end() {
        HIP_TRY(hipMemcpyAsync(cov.host.data(), cov.bins, cov.host.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        cov.host[0] += cov.init_generated;
        return MC_OK;
    }
    int coverage(mc_action_coverage *out, size_t *n_inout) override {
        if (!cov.on) { set_error("mc_engine_coverage: the engine was created without MC_F_COVERAGE"); return MC_ESTATE; }
        size_t n = 1;
        for (int a = 0; a + 1 < cov.nbins; a++) n += CovAction<S>::listed(prm, a) ? 1 : 0;
        if (n > *n_inout || !out) { *n_inout = n; set_error("mc_engine_coverage: buffer too small"); return MC_EBADCFG; }
        size_t k = 0;
        for (int a = -1; a + 1 < cov.nbins; a++) {
            if (a >= 0 && !CovAction<S>::listed(prm, a)) continue;
            out[k].action = a;
            out[k].pad = 0;
            out[k].generated = cov.host[(size_t)a + 1];
            out[k].distinct = cov.host[(size_t)cov.nbins + a + 1];
            k++;
        }
        *n_inout = n;
        return MC_OK;
    }

    // ------------------------------------------------------------------------------- the state graph (engine_graph.h)
    // All on `stream`, after a search has ended: rows, fingerprints and counters are final and only read.  The states with out-edges
    // are [0, fr.lo): run() moves `lo` past a level exactly when it has expanded it — the same (lo, hi) it hands to cov_generated —
    // so the levels coverage counts and the levels that have rows here cannot differ.
    template <class K, class... A>
    void graph_chunks(K kernel, uint64_t lo, uint64_t hi, A... args) {   // the chunks cov_generated launches
        each_chunk(lo, hi, [&](uint64_t c0, uint64_t c1, uint64_t ncols) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, stream, prm, (const uint64_t *)d_arena, c0, c1, ncols,
                               (const uint64_t *)d_table, seen_arg(), args...);
        });
    }
    int graph(mc_graph_info *out) override {
        memset(out, 0, sizeof *out);
        if (cfg.shard_count > 1) { set_error("mc_engine_graph: not available for a sharded engine (shard_count > 1)"); return MC_EBADCFG; }
        if (!fr.have_run || ck.pending) {
            set_error("mc_engine_graph: needs a search of this engine that returned a result (mc_engine_run / mc_engine_step; not a simulation, "
                      "not a restored checkpoint that has not run yet: its seen-set is not built)");
            return MC_ESTATE;
        }
        gr.release();
        gr.device = cfg.device;
        const uint64_t n = fr.last_distinct, expanded = fr.lo;
        if (n + 1 > 0x7fffffffull) { set_error("mc_engine_graph: at most 2^31 - 2 states (the scan's item count)"); return MC_EBADCFG; }
        HIP_TRY(hipSetDevice(cfg.device));
        const auto t0 = std::chrono::steady_clock::now();
        DevBuf<uint32_t> slot_index, degree;   // build-time only: gone when this call returns
        DevBuf<GraphCounters> d_gc;
        DevBuf<char> scan_tmp;
        int rc;
        if ((rc = graph_alloc(slot_index, table_cap, "the fingerprint -> state index"))) return rc;
        if ((rc = graph_alloc(degree, n + 1, "the out-degrees"))) return rc;
        if ((rc = graph_alloc(gr.offsets, n + 1, "the row offsets"))) { gr.release(); return rc; }
        if ((rc = graph_alloc(d_gc, 1, "the counters"))) { gr.release(); return rc; }
        const int built = graph_build(n, expanded, slot_index, degree, d_gc, scan_tmp);
        if (built) { gr.release(); return built; }
        gr.info.states = n;
        gr.info.expanded = expanded;
        gr.info.init_states = fr.level_start.size() > 1 ? fr.level_start[1] : n;
        gr.info.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        gr.built = true;
        *out = gr.info;
        return MC_OK;
    }
    int graph_build(uint64_t n, uint64_t expanded, DevBuf<uint32_t> &slot_index, DevBuf<uint32_t> &degree, DevBuf<GraphCounters> &d_gc, DevBuf<char> &scan_tmp) {
        GraphCounters gc;
        memset(&gc, 0, sizeof gc);
        gc.first_bad = ~0ull;
        HIP_TRY(hipMemcpyAsync(d_gc, &gc, sizeof gc, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(slot_index, 0xff, table_cap * sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(degree, 0, (n + 1) * sizeof(uint32_t), stream));
        if (n) hipLaunchKernelGGL(k_graph_index<S>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, prm, (const uint64_t *)d_arena, n,
                                  (const uint64_t *)d_table, seen_arg(), slot_index.p, table_cap, d_gc.p);
        graph_chunks(k_graph_degree<S>, 0, expanded, degree.p, d_gc.p);
        HIP_TRY(hipGetLastError());
        if (int rc = scan_exclusive_u32_to_u64(degree.p, gr.offsets.p, n + 1, scan_tmp, stream, "mc_engine_graph")) return rc;
        uint64_t edges = 0;
        HIP_TRY(hipMemcpyAsync(&edges, gr.offsets.p + n, sizeof edges, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&gc, d_gc, sizeof gc, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (int rc = graph_inconsistent(gc)) return rc;
        if (int rc = graph_alloc(gr.dst, edges, "the edges' successors")) return rc;
        if (int rc = graph_alloc(gr.act, edges, "the edges' actions")) return rc;
        graph_chunks(k_graph_fill<S>, 0, expanded, (const uint32_t *)slot_index.p, table_cap, (const uint64_t *)gr.offsets.p, gr.dst.p, gr.act.p, d_gc.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&gc, d_gc, sizeof gc, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (int rc = graph_inconsistent(gc)) return rc;
        gr.info.edges = edges;
        gr.info.self_loops = gc.self_loops;
        gr.info.dropped = gc.dropped;
        gr.info.max_out_degree = gc.max_degree;
        return MC_OK;
    }
    static int graph_inconsistent(const GraphCounters &gc) {
        if (!gc.missing_states && !gc.missing_succ) return MC_OK;
        const unsigned long long idx = gc.first_bad >> 16;
        const unsigned slot = (unsigned)(gc.first_bad & 0xffffu);
        set_error("mc_engine_graph: the seen-set does not hold " + std::to_string(gc.missing_states) + " stored state(s) and " + std::to_string(gc.missing_succ) +
                  " in-model successor(s); the first: state " + std::to_string(idx) + (slot == GRAPH_SLOT_SELF ? " itself" : ", slot " + std::to_string(slot)) +
                  " (two different states with one 64-bit fingerprint are the only legitimate cause: the second is never stored); no graph was built");
        return MC_ESTATE;
    }

    // ------------------------------------------------------------------------------- the predicates of the cfg's temporal properties
    // (LivePred<S>, k_live_pred<S>) and one (M, S, T) check over them
    int predicates_build(const char *call) {
        if constexpr (!LivePred<S>::HAS) {
            return MC_ENOSPEC;
        } else {
            auto &lv = gr.lv;
            if (lv.pred_built) return MC_OK;
            LivePredTab tab;
            memset(&tab, 0, sizeof tab);
            tab.n = vm_live_preds(prm.host, tab.entry, LIVE_MAX_PREDS);
            if (tab.n > LIVE_MAX_PREDS) { set_error(std::string(call) + ": at most 32 predicates"); return MC_EBADCFG; }
            const uint64_t n = gr.info.states;
            HIP_TRY(hipSetDevice(cfg.device));
            DevBuf<unsigned long long> d_bad;
            if (int rc = graph_alloc(lv.pred, n, "the predicate bits", call)) return rc;
            if (int rc = graph_alloc(d_bad, 1, "the counters", call)) return rc;
            unsigned long long bad = ~0ull;
            HIP_TRY(hipMemcpyAsync(d_bad, &bad, sizeof bad, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemsetAsync(lv.pred, 0, (n ? n : 1) * sizeof(uint32_t), stream));
            if (tab.n) graph_chunks(k_live_pred<S>, 0, n, tab, lv.pred.p, d_bad.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (bad != ~0ull) {
                lv.pred.reset();
                set_error(std::string(call) + ": evaluating the predicate `" + vm_live_pred_text(prm.host, (int)(bad & 0xff)) + "` fails in state " +
                          std::to_string(bad >> 8) + " (an evaluation error: a function applied outside its domain, an overflow, ...)");
                return MC_ESTATE;
            }
            lv.pred_built = true;
            lv.npred = tab.n;
            return MC_OK;
        }
    }
    int predicates(uint64_t first, uint64_t count, uint32_t *bits_out) override {
        if (cfg.shard_count > 1) { set_error("mc_engine_predicates: not available for a sharded engine (shard_count > 1)"); return MC_EBADCFG; }
        if constexpr (!LivePred<S>::HAS) {
            set_error("mc_engine_predicates: this lowering has no compiled predicates (compiled PlusCal programs only)");
            return MC_ENOSPEC;
        } else {
            if (!gr.built) { mc_graph_info gi; if (int rc = graph(&gi)) return rc; }
            if (int rc = predicates_build("mc_engine_predicates")) return rc;
            return gr.pred_read(first, count, bits_out);
        }
    }

    // ------------------------------------------------------------------------------- the liveness checks: the lowering's part (LiveProc<S>,
    // k_live_proc<S>, k_live_unit<S>) of all six C entries (DESIGN sections 16, 17, 19, 21).  Each entry fills a LiveQuery (live_query.h);
    // here, in ONE order: the outputs zeroed, the engine's conditions, the query's (live_query_error), what the graph lacks built —
    // components, the edges' processes or units, a property's predicates: once per graph, release() forgets them —, then
    // StateGraph::live_check.
    static_assert(LiveProc<S>::HAS == LivePred<S>::HAS, "a lowering with process instances compiles predicates, and no other does");
    DevBuf<int8_t> live_unit_tab;   // the program's (instance, label) -> unit table, as k_live_unit<S> reads it
    int liveness_run(const LiveQuery &query, const mc_live_property *prop, mc_live_info *out, mc_live_check_info *check_out, mc_live_strong_info *strong_out) override {
        LiveQuery q = query;
        const std::string call(q.call);
        auto t0 = std::chrono::steady_clock::now();
        if (out) memset(out, 0, sizeof *out);
        if (check_out) memset(check_out, 0, sizeof *check_out);
        if (strong_out) memset(strong_out, 0, sizeof *strong_out);
        if (cfg.shard_count > 1) { set_error(call + ": not available for a sharded engine (shard_count > 1)"); return MC_EBADCFG; }
        if constexpr (!LiveProc<S>::HAS) {
            set_error(call + ": this lowering has no process instances (compiled PlusCal programs only)");
            return MC_ENOSPEC;
        } else {
            if (!fr.have_run || ck.pending || fr.have_viol || fr.hi != fr.lo) {
                set_error(call + ": needs a search of this engine that finished without a violation and with an empty queue (the complete state graph)");
                return MC_ESTATE;
            }
            if (!q.fu) {
                const int np = LiveProc<S>::count(prm);
                if (np > LIVE_MAX_PROCS) { set_error(call + ": at most 64 process instances"); return MC_EBADCFG; }
                q.all = np >= 64 ? ~0ull : (1ull << np) - 1;
            }
            if (prop && prop->refused) { set_error(call + ": the front end refused " + prop->name); return MC_EBADCFG; }
            if (prop && q.term()) { set_error(call + ": " + live_unknown_kind(q.kind)); return MC_EBADCFG; }   // (-1 is no kind of a property)
            if (int rc = live_query_check(q, prop ? vm_live_preds(prm.host, nullptr, 0) : 0)) return rc;
            int ni = 0, nl = 0;
            if (q.fu) {   // (after the table's own conditions: a table with nunits < 0 is refused for that)
                const int nu = vm_live_units(prm.host, &ni, &nl, nullptr, 0);
                if (q.fu->nunits < nu) { set_error(call + ": the program has " + std::to_string(nu) + " units, the table " + std::to_string(q.fu->nunits)); return MC_EBADCFG; }
            }
            if (!gr.built || !gr.lv.scc_built) { mc_scc_info si; if (int rc = scc(&si)) return rc; }
            auto &lv = gr.lv;
            const uint64_t edges = gr.info.edges;
            HIP_TRY(hipSetDevice(cfg.device));
            if (!q.refine && !prop) t0 = std::chrono::steady_clock::now();   // (mc_engine_liveness's seconds leave the components out)
            if (!q.fu && !lv.proc_built) {
                if (int rc = graph_alloc(lv.proc, edges, "the edges' processes", q.call)) return rc;
                HIP_TRY(hipMemsetAsync(lv.proc, 0xff, (edges ? edges : 1) * sizeof(int8_t), stream));
                graph_chunks(k_live_proc<S>, 0, fr.lo, (const uint64_t *)gr.offsets.p, lv.proc.p);
                lv.proc_built = true;
            }
            if (q.fu && !lv.unit_built) {
                std::vector<int8_t> tab((size_t)ni * (size_t)nl + 1, (int8_t)LIVE_TERM);
                vm_live_units(prm.host, &ni, &nl, tab.data(), (int)tab.size());
                if (int rc = graph_alloc(live_unit_tab, tab.size(), "the units of the labels", q.call)) return rc;
                if (int rc = graph_alloc(lv.unit, edges, "the edges' units", q.call)) return rc;
                HIP_TRY(hipMemcpyAsync(live_unit_tab, tab.data(), tab.size() * sizeof(int8_t), hipMemcpyHostToDevice, stream));
                HIP_TRY(hipMemsetAsync(lv.unit, 0xff, (edges ? edges : 1) * sizeof(int8_t), stream));
                graph_chunks(k_live_unit<S>, 0, fr.lo, (const uint64_t *)gr.offsets.p, LiveUnitTab{ni, nl, (const int8_t *)live_unit_tab.p}, lv.unit.p);
                HIP_TRY(hipStreamSynchronize(stream));   // (the host table is read by the copy until here)
                lv.unit_built = true;
            }
            if (prop) if (int rc = predicates_build(q.call)) return rc;
            return gr.live_check(q, stream, t0, out, check_out, strong_out);
        }
    }

    template <class F>
    void timed(int which, uint64_t units, F &&launch, hipStream_t on = nullptr) {
        if (!timer.enabled) { launch(); return; }
        if (!on) on = stream;
        hipEvent_t a = timer.get(), b = timer.get();
        size_t ia = timer.used - 2, ib = timer.used - 1;
        hipEventRecord(a, on);
        launch();
        hipEventRecord(b, on);
        timer.pending.push_back({which, ia, ib, units});
    }

    int read_counters() {
        if (stream_b) HIP_TRY(hipStreamSynchronize(stream_b));
        HIP_TRY(hipStreamSynchronize(stream2));
        HIP_TRY(hipMemcpyAsync(h_ctr, d_ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (timer.enabled) timer.resolve(kstat);
        return MC_OK;
    }
    int check_dev_error() {
        if (h_ctr->error & DEV_EOVERFLOW) { set_error("packed-state capacity exceeded (raft messages / elections / allLogs slots, or a PlusCal sequence longer than its cells, or a recursive PlusCal procedure deeper than $TLAMC_PCAL_STACK frames)"); return MC_EOVERFLOW; }
        if (h_ctr->error & DEV_ETABLE) { set_error("seen-set full: raise table_capacity"); return MC_ETABLEFULL; }
        if (h_ctr->error & DEV_EROUTE) { set_error("sharded round: an exchange bucket is full (raise the fan-out allowance / send capacity)"); return MC_EROUTE; }
        if (h_ctr->error & DEV_EARENA) { set_error("state arena full: raise arena_capacity"); return MC_EARENA; }
        return MC_OK;
    }

    bool inwave_ok() const { return (UsesFamilies<S>::value || UsesPairs<S>::value) && !use_matrix && !(cfg.flags & (MC_F_NOFAMILY | MC_F_NOINWAVE)); }
    // by-pairs specs (engine_pairs.h) write EVERY new state in the expand kernel: nothing ever reaches the new-list, so a fused run launches
    // neither k_materialise nor k_commit for them
    bool pairs_only() const { return UsesPairs<S>::value && inwave_ok(); }
    void set_inwave(RouteArgs &rt) const {
        if (!inwave_ok()) return;
        rt.arena_w = d_arena;
        rt.arena_cap = arena_cap;
        rt.parent = d_parent;
        rt.pslot = d_pslot;
    }
    // k_materialise's grid (x NSHARD segments) for the new-list of a chunk of ncols parents (a grid-stride kernel: any grid is correct)
    static unsigned mat_grid(uint64_t ncols) {
        const unsigned bx = (unsigned)((ncols + 255) / 256);
        const unsigned gm = bx < 8 * 256 ? (bx + 7) / 8 : 256;
        return gm ? gm : 1u;
    }
    // materialise + commit of the chunk whose survivors are in new-list `parity`, on the second stream: it overlaps
    // the expansion of the next chunk (memory-bound next to latency-bound)
    void finish_materialise(uint64_t chunk_base, uint64_t ncols, unsigned parity, hipStream_t expanded_on = nullptr) {
        if (pairs_only()) return;
        unsigned gm = mat_grid(ncols);
        // In-wave levels hand k_materialise only the OVERFLOW of the expand wavefronts' survivor lists (0.15 % of the contract workload's
        // states, 11 % of the five-server model's): the grid follows what the level before sent through the list (x 4, per chunk) instead
        // of the chunk's size — a grid-stride kernel: any grid is correct — so that a launch with next to nothing to do is 8 workgroups
        // that start and end at once, not 2048 that queue behind the next chunk's expand (round 5: 70 launches per step showed 62 ms of
        // HIP-event time for 0.8 M states: VERDICT weak 9)
        if (fr.mat_inwave_level) {
            const uint64_t want = (fr.mat_list_hint * 4 + 255) / 256;   // workgroups of 256 states, all eight segments together
            const unsigned per_seg = (unsigned)((want + NSHARD - 1) / NSHARD);
            if (per_seg < gm) gm = per_seg ? per_seg : 1u;
        }
        hipEventRecord(ev_e[parity].get(), expanded_on ? expanded_on : stream.s);
        hipStreamWaitEvent(stream2, ev_e[parity].get(), 0);
        timed(2, 0, [&] {
            hipLaunchKernelGGL(k_materialise<S>, dim3(gm, NSHARD), dim3(256), 0, stream2, prm, d_arena, chunk_base, d_newlist,
                               seg_cap, arena_cap, d_parent, d_pslot, d_ctr, parity, (const LevelCtl *)nullptr, (const uint64_t *)d_newfp);
        }, stream2);
        hipLaunchKernelGGL(k_commit, dim3(1), dim3(1), 0, stream2, d_ctr, parity);
        hipEventRecord(ev_m[parity].get(), stream2);
        // measurement knob: TLAMC_SERIAL=1 lets no expand kernel run beside a materialise kernel (each kernel's stand-alone time)
        static const bool serial = getenv("TLAMC_SERIAL") != nullptr;
        if (serial) hipStreamSynchronize(stream2);
    }
    // one batched level (LevelCtl): the same pair of kernels, ranges read on the device, then the level is closed there
    void enqueue_blind_level(uint64_t max_states) {
        // all four kernels on ONE stream: for a frontier this small the two-stream overlap buys nothing and the
        // cross-stream events would cost more than the kernels
        const uint64_t ncols = max_states + 64;
        RouteArgs rt{};
        rt.lc = d_lc;
        rt.new_fp = d_newfp;
        set_inwave(rt);
        const unsigned sg = slices_for(ncols, true);
        const bool dl = sg > 1 && (cfg.flags & MC_F_DEADLOCK);
        if (dl) { rt.succ = d_nsl; hipMemsetAsync(d_nsl, 0, ncols * sizeof(uint16_t), stream); }
        const unsigned lflags = cfg.flags | ((cfg.flags & MC_F_PARK) ? MC_FI_PARK : 0u);   // (the PARK instantiation, see run())
        timed(0, 0, [&] {
            launch_expand<S, false>(!(cfg.flags & MC_F_NOFAMILY), lflags, ncols, stream, sg, prm, (const uint64_t *)d_arena,
                                    (uint64_t)0, (uint64_t)0, ncols, d_table.p, seen_arg(), d_newlist.p, seg_cap, d_ctr.p, cfg.flags, rt, 0u);
            if (dl) hipLaunchKernelGGL(k_deadlock_slices, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, stream, (const uint16_t *)d_nsl,
                                       (uint64_t)0, (uint64_t)0, ncols, (const LevelCtl *)d_lc, d_ctr);
        });
        if (!pairs_only()) timed(2, 0, [&] {
            hipLaunchKernelGGL(k_materialise<S>, dim3(32, NSHARD), dim3(256), 0, stream, prm, d_arena, (uint64_t)0, d_newlist, seg_cap,
                               arena_cap, d_parent, d_pslot, d_ctr, 0u, (const LevelCtl *)d_lc, (const uint64_t *)d_newfp);
        });
        hipLaunchKernelGGL(k_end_level, dim3(1), dim3(1), 0, stream, d_ctr, d_lc);
    }

    // insert + materialise + commit for the candidate matrix just written
    template <bool INIT>
    void finish_chunk(uint64_t chunk_base_or_first, uint64_t ncols, unsigned rows) {
        const unsigned bx = (unsigned)((ncols + 255) / 256);
        timed(1, ncols * rows, [&] {
            hipLaunchKernelGGL(k_insert, dim3(bx, rows), dim3(256), 0, stream, d_cand, row_stride, ncols, d_nsl, d_table,
                               seen_arg(), d_newlist, d_ctr);
        });
        const unsigned gm = bx < 2048 ? bx : 2048;
        timed(2, 0, [&] {
            if (INIT)
                hipLaunchKernelGGL(k_init_materialise<S>, dim3(gm), dim3(256), 0, stream, prm, d_arena, chunk_base_or_first,
                                   d_inittmp, d_newlist, arena_cap, d_parent, d_pslot, d_ctr);
            else
                hipLaunchKernelGGL(k_materialise<S>, dim3(gm, 1), dim3(256), 0, stream, prm, d_arena, chunk_base_or_first,
                                   d_newlist, seg_cap, arena_cap, d_parent, d_pslot, d_ctr, 0u, (const LevelCtl *)nullptr, (const uint64_t *)nullptr);
        });
        hipLaunchKernelGGL(k_commit, dim3(1), dim3(1), 0, stream, d_ctr, 0u);
    }

    // The start of every search, on `stream`: an empty seen-set, fresh counters, then level 1 = the initial states that `rank` of `count`
    // owns.  resuming (run() after restore() / inside step()): the counters are the handed-over run's and its states are in the arena
    // already; the seen-set is rebuilt from them unless it is still valid (in_place).  t0 (fused runs): the run's clock starts when the
    // clearing is done, before the first kernel is enqueued.
    int seed_init(unsigned rank, unsigned count, bool resuming, bool in_place, std::chrono::steady_clock::time_point *t0) {
        if (!in_place) HIP_TRY(hipMemsetAsync(d_table, 0, table_cap * sizeof(uint64_t), stream));
        HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(DevCounters), stream));
        DevCounters init_c;
        memset(&init_c, 0, sizeof init_c);
        init_c.viol_key = ~0ull;
        if (resuming) {
            init_c.arena_next = ck.distinct;
            init_c.generated[0].v = ck.generated;
            init_c.cells[0].v = ck.cells;
        }
        HIP_TRY(hipMemcpyAsync(d_ctr, &init_c, sizeof init_c, hipMemcpyHostToDevice, stream));
        if (t0) {
            HIP_TRY(hipStreamSynchronize(stream));
            *t0 = std::chrono::steady_clock::now();
        }
        if (resuming && ck.distinct && !in_place)
            hipLaunchKernelGGL(k_reseed_table<S>, dim3((unsigned)((ck.distinct + 255) / 256)), dim3(256), 0, stream, prm,
                               (const uint64_t *)d_arena, ck.distinct, d_table, seen_arg(), d_ctr);
        const uint64_t ninit = resuming ? 0 : S::num_init(prm);
        for (uint64_t first = 0; first < ninit; first += chunk) {
            const uint64_t n = ninit - first < chunk ? ninit - first : chunk;
            const uint64_t ncols = (n + 63) & ~63ull;
            hipLaunchKernelGGL(k_init_cand<S>, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, stream, prm, first, n,
                               d_inittmp, d_cand, ncols, d_nsl, d_ctr, rank, count);
            finish_chunk<true>(first, ncols, 1);
        }
        return MC_OK;
    }
    // The level [lo, hi) has been expanded and the arena now ends at new_hi: the next frontier is [hi, new_hi), a level of its own
    // unless it is empty.
    int close_level(uint64_t &lo, uint64_t &hi, uint64_t new_hi, uint32_t &level, mc_result *out) {
        lo = hi;
        hi = new_hi;
        if (hi > lo) {
            fr.level_start.push_back(lo);
            if (level < MC_MAX_LEVELS) out->level_distinct[level] = hi - lo;
            level++;
        }
        if (level >= MC_MAX_LEVELS) { set_error("too many BFS levels"); return MC_EBADCFG; }
        return MC_OK;
    }

    int run(mc_result *out) override {
        memset(out, 0, sizeof *out);
        out->violated_invariant = -1;
        memset(kstat, 0, sizeof kstat);
        fr.have_viol = false;
        sim.trace_n = 0;
        stop_requested = false;
        gr.release();
        fr.have_run = false;  // set again on the success path only: a run that fails half-way (MC_EARENA, MC_ETABLEFULL, MC_EOVERFLOW)
                           // leaves fingerprints of an unfinished level in the seen-set — the next step / checkpoint must not continue it
        fr.level_start.clear();
        HIP_TRY(hipSetDevice(cfg.device));
        const bool resuming = ck.pending, in_place = ck.pending && ck.in_place;  // in place (mc_engine_step): the seen-set of the stopped run is still valid
        ck.pending = ck.in_place = false;
        std::chrono::steady_clock::time_point t0;
        int rc = seed_init(0u, 1u, resuming, in_place, &t0);  // level 1: Init; run() is never owner-filtered
        if (rc) return rc;
        progress_last = t0;
        auto progress = [&](uint32_t lv, uint64_t lo_, uint64_t hi_) {
            if (!progress_fn) return;
            uint64_t g = 0;
            for (int t = 0; t < NSHARD; t++) g += h_ctr->generated[t].v;
            report_progress(lv, g, hi_, hi_ - lo_);
        };
        // with in-wave writes every writer takes its arena indices from arena_next itself from here on (DevCounters::atomic_alloc).
        // Init above, the candidate-matrix form and every spec whose states all go through k_materialise keep appending in stream
        // order: one returning atomicAdd per wavefront of k_materialise on ONE word is pure cost there (atomic_add N = 28: 145
        // against 108 ms per run, profiles/r04h / r04i; raft through k_materialise only: 203 against 159 ms)
        if (inwave_ok()) hipLaunchKernelGGL(k_set_alloc_mode, dim3(1), dim3(1), 0, stream, d_ctr, 1u);
        bool alloc_atomic = inwave_ok();
        uint64_t prev_frontier = ~0ull >> 12;  // (the first level is never "fast growing")
        if ((rc = read_counters())) return rc;
        if ((rc = check_dev_error())) return rc;
        uint64_t lo = 0, hi = h_ctr->arena_next;
        uint32_t level = 1;
        out->level_distinct[0] = hi;
        fr.level_start.push_back(0);
        // (a step that continues in place keeps counting; every other search starts its counts over)
        if (cov.on && !in_place && (rc = cov_begin(resuming ? ck.lo : 0, hi))) return rc;
        if (vio.on) {   // (a search that is continued has found nothing so far: its tables start empty either way)
            if ((rc = viol_begin())) return rc;
            if (!resuming && h_ctr->viol_key != ~0ull && (rc = viol_level(0, hi, hi, false))) return rc;   // Init breaks an invariant
        }
        if (resuming) {  // continue with the frontier [lo, hi) = the last, unexpanded level of the checkpointed run
            fr.level_start = ck.level_start;
            level = (uint32_t)fr.level_start.size();
            lo = ck.lo;
            for (uint32_t k = 0; k < level && k < MC_MAX_LEVELS; k++)
                out->level_distinct[k] = (k + 1 < level ? fr.level_start[k + 1] : hi) - fr.level_start[k];
        }
        int budget = 0;
        uint64_t via_seen = 0;
        // PARKING (round 6, MC_F_PARK): the instantiation of the by-family kernel whose writers park the overflow of their survivor lists and
        // write it themselves (k_expand_family<.., PARK>).  Measured (profiles/r06zb, zf, zg, zh): every state of the five-server model
        // is written in-wave then (924 M instead of 821 M; k_materialise idle) and its step takes as long as before, or longer — not the default
        const bool park_levels = (cfg.flags & MC_F_PARK) != 0;
        fr.mat_list_hint = ~0ull >> 8;   // (unknown before the first large level: the full grid)
        fr.mat_inwave_level = false;
        // (the largest frontier a batched level takes: 2^20 states since round 6 — 2^16 before; profiles/r06zm_blind_ab.jsonl: the contract
        //  workload 128.7 / 127.5 -> 126.1 / 126.0 ms, the generated pagecache model 7.65 / 7.63 -> 7.42 / 7.44 — $TLAMC_BLIND_LOG2 = A/B knob.
        //  Specs whose blind launches are sliced — the interpreter, the Paxos family: 32 slices of the level's CAPACITY — keep 2^16)
        static const int blind_log2 = getenv("TLAMC_BLIND_LOG2") ? atoi(getenv("TLAMC_BLIND_LOG2")) : 20;
        uint64_t blind_max = 1ull << (blind_log2 >= 10 && blind_log2 <= 23 && slices_for((1ull << 16) + 64, true) == 1 ? blind_log2 : 16);
        if (chunk < blind_max) blind_max = chunk;
        while (hi > lo) {
            if (h_ctr->viol_key != ~0ull) break;
            if (fr.stop_frontier && hi - lo >= fr.stop_frontier) break;  // the caller continues this level sharded
            if (cfg.max_levels && level >= cfg.max_levels) { budget = 1; break; }
            if (cfg.max_distinct && hi >= cfg.max_distinct) { budget = 1; break; }
            if (stop_requested) { budget = 1; break; }
            if (!use_matrix && !(cfg.flags & MC_F_NOBATCH) && hi - lo <= blind_max) {
                // Small frontier: BLIND_BATCH levels are enqueued back to back; the kernels take each level's range from
                // LevelCtl and k_end_level applies the same stopping rules as this loop, so one host round trip covers
                // up to BLIND_BATCH levels instead of one (a level of a few thousand states is pure launch latency).
                memset(h_lc, 0, sizeof(LevelCtl));
                h_lc->lo = lo;
                h_lc->hi = hi;
                // (a replicated prefix ends BEFORE the first level of stop_frontier states, inside a batch too: k_end_level leaves a batch
                //  at a level of more than max_states, so that level is the one the loop head hands to the sharded rounds)
                h_lc->max_states = fr.stop_frontier && fr.stop_frontier - 1 < blind_max ? fr.stop_frontier - 1 : blind_max;
                h_lc->max_distinct = cfg.max_distinct;
                h_lc->levels_left = cfg.max_levels ? (unsigned)(cfg.max_levels - level) : 0u;
                HIP_TRY(hipMemcpyAsync(d_lc, h_lc, sizeof(LevelCtl), hipMemcpyHostToDevice, stream));
                HIP_TRY(hipStreamSynchronize(stream2));  // (nothing of an earlier level is still being materialised)
                if (inwave_ok() && !alloc_atomic) {  // the batched small levels always write in-wave
                    hipLaunchKernelGGL(k_set_alloc_mode, dim3(1), dim3(1), 0, stream, d_ctr, 1u);
                    alloc_atomic = true;
                }
                for (int k = 0; k < BLIND_BATCH; k++) enqueue_blind_level(blind_max);
                HIP_TRY(hipMemcpyAsync(h_lc, d_lc, sizeof(LevelCtl), hipMemcpyDeviceToHost, stream));
                if ((rc = read_counters())) return rc;
                if ((rc = check_dev_error())) return rc;
                for (unsigned k = 0; k < h_lc->nlev; k++) {
                    kstat[0].units += hi - lo;  // states expanded by this level (the launches were timed with 0 units)
                    if (cov.on) { cov_generated(lo, hi); cov_distinct(hi, h_lc->level_hi[k]); }
                    // (k_end_level stops a batch at its first flagged level: the key is that of the last level it completed)
                    if (vio.on && k + 1 == h_lc->nlev && h_ctr->viol_key != ~0ull && (rc = viol_level(lo, hi, h_lc->level_hi[k], true))) return rc;
                    if ((rc = close_level(lo, hi, h_lc->level_hi[k], level, out))) return rc;
                }
                progress(level, lo, hi);
                prev_frontier = hi > lo ? hi - lo : 1;
                continue;  // the loop head re-checks violation / budgets / frontier with the host's copies
            }
            // IN-WAVE WRITES, level by level (inwave_growth_limit above: a level that grows faster than the limit goes through the
            // new-list and k_materialise alone).  The level before this one says which kind it is; the allocation mode
            // (DevCounters::atomic_alloc) follows — nothing is in flight between two levels.
            const bool lvl_inwave = inwave_ok() && (pairs_only() || (double)(hi - lo) <= inwave_growth_limit * (double)prev_frontier);
            if (inwave_ok() && lvl_inwave != alloc_atomic) {
                hipLaunchKernelGGL(k_set_alloc_mode, dim3(1), dim3(1), 0, stream, d_ctr, lvl_inwave ? 1u : 0u);
                alloc_atomic = lvl_inwave;
            }
            prev_frontier = hi - lo;
            fr.mat_inwave_level = lvl_inwave;
            unsigned chunk_no = 0;
            // (odd chunks on their own stream — see stream_b; not with the slot-sliced launches' shared flag array, not for the matrix form)
            const bool two_streams = stream_b && !use_matrix && hi - lo > chunk && !(slices_for(chunk, false) > 1 && (cfg.flags & MC_F_DEADLOCK));
            if (two_streams) {  // what the level's first kernels on `stream` were ordered behind, stream_b's are too
                hipEventRecord(ev_level.get(), stream);
                hipStreamWaitEvent(stream_b, ev_level.get(), 0);
            }
            for (uint64_t c0 = lo; c0 < hi; ++chunk_no) {
                const unsigned parity = chunk_no & 1u;
                const uint64_t base = c0 & ~63ull;
                uint64_t c1 = base + chunk;  // chunk boundaries stay 64-aligned
                if (c1 > hi) c1 = hi;
                const uint64_t ncols = ((c1 - base) + 63) & ~63ull;
                if (use_matrix) {  // two-kernel form: sparse candidate matrix + k_insert (kept for A/B measurements)
                    timed(0, c1 - c0, [&] {
                        hipLaunchKernelGGL(k_expand<S>, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, stream, prm, d_arena,
                                           c0, c1, d_cand, row_stride, ncols, d_nsl, d_ctr, cfg.flags);
                    });
                    finish_chunk<false>(base, ncols, max_slots);
                } else {
                    hipStream_t es = two_streams && parity ? stream_b.s : stream.s;
                    if (chunk_no >= 2) hipStreamWaitEvent(es, ev_m[parity].get(), 0);  // new-list `parity` is free again
                    RouteArgs rt_new{};
                    rt_new.new_fp = d_newfp;
                    if (lvl_inwave) set_inwave(rt_new);
                    const unsigned sg = slices_for(ncols, false);
                    const bool dl = sg > 1 && (cfg.flags & MC_F_DEADLOCK);
                    if (dl) { rt_new.succ = d_nsl; hipMemsetAsync(d_nsl, 0, ncols * sizeof(uint16_t), es); }
                    const unsigned lflags = cfg.flags | (lvl_inwave && park_levels ? MC_FI_PARK : 0u);
                    timed(0, c1 - c0, [&] {
                        launch_expand<S, false>(!(cfg.flags & MC_F_NOFAMILY), lflags, ncols, es, sg, prm,
                                                (const uint64_t *)d_arena, c0, c1, ncols, d_table.p, seen_arg(), d_newlist.p, seg_cap, d_ctr.p,
                                                cfg.flags, rt_new, parity);
                        if (dl) hipLaunchKernelGGL(k_deadlock_slices, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, es,
                                                   (const uint16_t *)d_nsl, c0, c1, ncols, (const LevelCtl *)nullptr, d_ctr);
                    }, es);
                    finish_materialise(base, ncols, parity, es);
                }
                c0 = c1;
            }
            if ((rc = read_counters())) return rc;
            if ((rc = check_dev_error())) return rc;
            {   // what this level sent through the new-list, per chunk, scaled by the level's growth: the next level's k_materialise grid
                const uint64_t via = h_ctr->via_list - via_seen;
                via_seen = h_ctr->via_list;
                const double growth = hi > lo ? (double)(h_ctr->arena_next - hi) / (double)(hi - lo) : 1.0;
                fr.mat_list_hint = (uint64_t)((double)(via / (chunk_no ? chunk_no : 1u)) * (growth > 1.0 ? growth : 1.0)) + 1;
            }
            if (cov.on) { cov_generated(lo, hi); cov_distinct(hi, h_ctr->arena_next); }
            if (vio.on && h_ctr->viol_key != ~0ull && (rc = viol_level(lo, hi, h_ctr->arena_next, true))) return rc;
            if ((rc = close_level(lo, hi, h_ctr->arena_next, level, out))) return rc;
            progress(level, lo, hi);
        }
        if (cov.on && (rc = cov_end())) return rc;
        // a run that stops with an unexpanded frontier (budget) has not evaluated that level's check-on-expand invariants yet
        if (hi > lo && h_ctr->viol_key == ~0ull && !fr.stop_frontier && (rc = check_frontier(lo, hi))) return rc;
        if (vio.on && hi > lo && !vio.fatal && h_ctr->viol_key != ~0ull && (rc = viol_level(lo, hi, hi, false))) return rc;   // ... and counted
        // -continue: the run reports its FIRST flagged level, whatever came after it
        const unsigned long long run_key = vio.on && vio.have_first ? vio.first_key : h_ctr->viol_key;
        const auto t1 = std::chrono::steady_clock::now();
        out->seconds = std::chrono::duration<double>(t1 - t0).count();
        out->distinct = h_ctr->arena_next;
        fr.last_distinct = h_ctr->arena_next;
        kstat[2].units = h_ctr->arena_next;
        out->generated = 0;
        fr.cells = 0;
        for (int t = 0; t < NSHARD; t++) { out->generated += h_ctr->generated[t].v; fr.cells += h_ctr->cells[t].v; }
        fr.last_generated = out->generated;
        // (a resumed run counts from the checkpoint on: via_list starts at 0 there)
        fr.inwave = inwave_ok() && h_ctr->arena_next >= h_ctr->via_list + (resuming ? ck.distinct : 0)
                           ? h_ctr->arena_next - h_ctr->via_list - (resuming ? ck.distinct : 0) : 0;  // (Init's states went through the list too)
        fr.have_run = true;
        out->queue_left = hi - lo;
        out->depth = level;
        out->levels = level;
        fr.lo = lo;
        fr.hi = hi;
        if (run_key != ~0ull) {
            fr.have_viol = true;
            fr.last_viol = run_key;
            const Viol v(fr.last_viol);
            out->verdict = v.verdict;
            out->violated_invariant = v.invariant;
            std::vector<uint64_t> chain;
            if (build_chain(chain) == MC_OK) out->trace_len = (uint32_t)chain.size() + (v.extra_state() ? 1u : 0u);
        } else {
            out->verdict = budget ? MC_V_BUDGET : MC_V_OK;
        }
        return MC_OK;
    }

    // ------------------------------------------------------------------------------- checkpoint / recover
    // TLC checkpoints a run into its states/ directory and continues it with -recover (testout1:10: "-- Checkpointing of
    // run states/01-08-03-18-14-01 completed."; .gitignore:2).  Here the resident arena already IS the state store: a
    // checkpoint is the arena's used blocks as they lie in HBM, the level boundaries, the counters and (with MC_F_TRACE)
    // the parent pointers.  The seen-set is not written: recovery re-inserts word 0 of every state (k_reseed_table).
    // mc_engine_step: `levels` more BFS levels.  The first call (or a call after a run that ended: complete, or with an error)
    // starts from Init; a call after a budget stop continues IN PLACE — arena, seen-set and parent pointers stay where they
    // are in HBM, only the counters and the level table are handed over (the same hand-over as restore(), without the file
    // and without rebuilding the seen-set).
    int step(uint32_t levels, mc_result *out) override {
        if (!levels) return MC_EBADCFG;
        const uint64_t saved = cfg.max_levels;
        const bool cont = fr.have_run && !fr.have_viol && fr.hi > fr.lo && !ck.pending;
        if (cont) {
            ck.distinct = fr.last_distinct; ck.generated = fr.last_generated; ck.cells = fr.cells; ck.lo = fr.lo;
            ck.level_start = fr.level_start;
            ck.pending = ck.in_place = true;
            cfg.max_levels = (uint64_t)fr.level_start.size() + levels;
        } else if (ck.pending) {  // restore() handed a checkpoint over: `levels` more levels beyond the checkpointed ones
            cfg.max_levels = (uint64_t)ck.level_start.size() + levels;
        } else {
            cfg.max_levels = levels;
        }
        const int rc = run(out);
        cfg.max_levels = saved;
        if (rc) ck.pending = ck.in_place = false;  // after a failure the next step starts over
        return rc;
    }
    // ---- the codec both formats share (CkIdent .. CkPart above)
    bool ck_params_comparable() const { return desc.spec_id != MC_SPEC_PCAL; }  // a compiled program's parameter is a host pointer
    void ck_fill_ident(CkIdent &id, const CkFormat &fmt) const {
        memcpy(id.magic, fmt.magic, 8);
        id.spec_id = desc.spec_id;
        id.nparams = ck_params_comparable() ? desc.nparams : 1;
        for (uint32_t i = 0; i < id.nparams && i < 16; i++) id.params[i] = desc.params[i];
        if (!ck_params_comparable()) id.params[0] = (int64_t)program_hash;  // a compiled program is identified by its image
        id.words = (uint32_t)W;
        id.has_trace = d_parent ? 1u : 0u;
    }
    static int ck_fail(int code, const char *who, const std::string &msg) { set_error(std::string(who) + ": " + msg); return code; }
    int ck_check_ident(const CkIdent &id, const CkFormat &fmt) const {
        if (memcmp(id.magic, fmt.magic, 8) != 0) return ck_fail(MC_EPARSE, fmt.reader, fmt.not_ours);
        if (id.spec_id != desc.spec_id || id.words != (uint32_t)W) return ck_fail(MC_EBADCFG, fmt.reader, "the checkpoint belongs to another spec");
        if (ck_params_comparable() && (id.nparams != desc.nparams || memcmp(id.params, desc.params, sizeof(int64_t) * (id.nparams < 16 ? id.nparams : 16)) != 0))
            return ck_fail(MC_EBADCFG, fmt.reader, "the checkpoint was written with other constants / invariants");
        if (!ck_params_comparable() && (id.nparams != 1 || (uint64_t)id.params[0] != program_hash)) return ck_fail(MC_EBADCFG, fmt.reader, fmt.other_program);
        return MC_OK;
    }
    // the device sections of a checkpoint of the first n states of the arena, in file order; per_rank: + parent ranks and the seen-set slice
    std::vector<CkPart> ck_sections(uint64_t n, bool per_rank) const {
        std::vector<CkPart> v{{d_arena.p, (size_t)((n + 63) >> 6) * (size_t)W * 64 * sizeof(uint64_t)}};
        if (d_parent) {
            v.push_back({d_parent.p, (size_t)n * sizeof(uint32_t)});
            v.push_back({d_pslot.p, (size_t)n * sizeof(uint16_t)});
        }
        if (per_rank && d_prank) v.push_back({d_prank.p, (size_t)n});
        if (per_rank) v.push_back({d_table.p, (size_t)table_cap * sizeof(uint64_t)});
        return v;
    }
    // the whole file: the host parts (header, level table, ...), then the device sections
    int ck_write(const CkFormat &fmt, const char *path, std::initializer_list<CkPart> host, const std::vector<CkPart> &dev) {
        FILE *f = fopen(path, "wb");
        if (!f) return ck_fail(MC_EBADCFG, fmt.writer, std::string("cannot write ") + path);
        FileCloser closer{f};  // early returns (HIP errors) must not leak the handle
        int rc = MC_OK;
        for (const CkPart &h : host)
            if (!rc && fwrite(h.p, 1, h.bytes, f) != h.bytes) rc = ck_fail(MC_EBADCFG, fmt.writer, "short write");
        for (const CkPart &d : dev) {
            if (rc) break;
            std::vector<char> buf(d.bytes < (64u << 20) ? d.bytes : (64u << 20));
            for (size_t off = 0; off < d.bytes && !rc; off += buf.size()) {
                const size_t n = d.bytes - off < buf.size() ? d.bytes - off : buf.size();
                HIP_TRY(hipMemcpy(buf.data(), (const char *)d.p + off, n, hipMemcpyDeviceToHost));
                if (fwrite(buf.data(), 1, n, f) != n) rc = ck_fail(MC_EBADCFG, "checkpoint", "short write");
            }
        }
        closer.f = nullptr;
        if (fclose(f) != 0 && !rc) rc = ck_fail(MC_EBADCFG, fmt.writer, "close failed");
        return rc;
    }
    // reading goes in three steps, the caller's own checks between them: header (read, identity checked), host parts, sections
    template <class H>
    int ck_read_header(const CkFormat &fmt, FILE *f, H &h) const {
        if (fread(&h, sizeof h, 1, f) != 1) return ck_fail(MC_EPARSE, fmt.reader, fmt.not_ours);
        return ck_check_ident(h.id, fmt);
    }
    static int ck_read_host(const CkFormat &fmt, FILE *f, std::initializer_list<CkPart> host) {
        for (const CkPart &h : host)
            if (fread(h.p, 1, h.bytes, f) != h.bytes) return ck_fail(MC_EPARSE, fmt.reader, "the checkpoint file is truncated");
        return MC_OK;
    }
    static int ck_read_sections(FILE *f, const std::vector<CkPart> &dev) {
        for (const CkPart &d : dev) {
            std::vector<char> buf(d.bytes < (64u << 20) ? d.bytes : (64u << 20));
            for (size_t off = 0; off < d.bytes; off += buf.size()) {
                const size_t n = d.bytes - off < buf.size() ? d.bytes - off : buf.size();
                if (fread(buf.data(), 1, n, f) != n) return ck_fail(MC_EPARSE, "restore", "the checkpoint file is truncated");
                HIP_TRY(hipMemcpy((char *)d.p + off, buf.data(), n, hipMemcpyHostToDevice));
            }
        }
        return MC_OK;
    }
    int checkpoint(const char *path) override {
        if (cfg.shard_count > 1) { set_error("checkpoint: not available for a sharded engine"); return MC_EBADCFG; }
        if (!fr.have_run || fr.have_viol) { set_error("checkpoint: needs a completed mc_engine_run that stopped on a budget (or finished) without a violation"); return MC_EBADCFG; }
        HIP_TRY(hipSetDevice(cfg.device));
        HIP_TRY(hipDeviceSynchronize());
        CkHeader h;
        memset(&h, 0, sizeof h);
        ck_fill_ident(h.id, CK_FUSED);
        h.distinct = fr.last_distinct; h.generated = fr.last_generated; h.cells = fr.cells;
        h.lo = fr.lo; h.hi = fr.hi; h.nlevels = fr.level_start.size();
        return ck_write(CK_FUSED, path, {{&h, sizeof h}, {fr.level_start.data(), fr.level_start.size() * sizeof(uint64_t)}}, ck_sections(fr.last_distinct, false));
    }
    int restore(const char *path) override {
        if (cfg.shard_count > 1) { set_error("restore: not available for a sharded engine"); return MC_EBADCFG; }
        gr.release();
        FileCloser f{fopen(path, "rb")};
        if (!f.f) return ck_fail(MC_EPARSE, "restore", std::string("cannot read ") + path);
        CkHeader h;
        int rc = ck_read_header(CK_FUSED, f.f, h);
        if (rc) return rc;
        // a run may legitimately stop on a budget at a seen-set load of 0.5 - 0.8 (the bench model at 2^27 slots ends at 0.76): its
        // checkpoint must restore into the same configuration; beyond 0.9 the reseeding itself could not finish (DEV_ETABLE)
        if (h.distinct * 10 > table_cap * 9) return ck_fail(MC_ETABLEFULL, "restore", "table_capacity cannot hold the checkpoint's states (load > 0.9)");
        if (h.distinct > arena_cap) return ck_fail(MC_EARENA, "restore", "arena_capacity is smaller than the checkpoint");
        if (h.hi != h.distinct || h.lo > h.hi || h.nlevels == 0 || h.nlevels >= MC_MAX_LEVELS) return ck_fail(MC_EPARSE, "restore", "inconsistent header");
        if (d_parent && !h.id.has_trace) return ck_fail(MC_EBADCFG, "restore", "the checkpoint holds no parent pointers (written without MC_F_TRACE); run without MC_F_TRACE");
        ck.level_start.assign((size_t)h.nlevels, 0);
        if ((rc = ck_read_host(CK_FUSED, f.f, {{ck.level_start.data(), ck.level_start.size() * sizeof(uint64_t)}}))) return rc;
        // level table: starts at 0, strictly increasing, below the fill level; an unexpanded frontier IS the last level
        bool ok = ck.level_start[0] == 0 && ck.level_start.back() < h.hi && (h.lo == h.hi || ck.level_start.back() == h.lo);
        for (size_t k = 1; k < ck.level_start.size() && ok; k++) ok = ck.level_start[k] > ck.level_start[k - 1];
        if (!ok) return ck_fail(MC_EPARSE, "restore", "inconsistent level table");
        HIP_TRY(hipSetDevice(cfg.device));
        if ((rc = ck_read_sections(f.f, ck_sections(h.distinct, false)))) return rc;
        ck.distinct = h.distinct; ck.generated = h.generated; ck.cells = h.cells; ck.lo = h.lo;
        ck.pending = true;  // the next run() continues from here
        return MC_OK;
    }
    // One checkpoint file per rank (testout1:10).
    // A rank's share of a sharded run cannot be rebuilt from its arena alone: the states a rank HOLDS are the ones it generated
    // (stay levels) or was sent (move levels), the fingerprints its seen-set slice holds are the ones it OWNS.  So a rank's file is
    // its arena, its parent pointers (index, slot, rank), its seen-set slice as it lies in HBM, its counters, and the level table of
    // the whole job (the same on every rank; the level loop hands it over when a run ends: shard_note_levels).  Restoring needs
    // the same world size, rank, table_capacity and spec; the next mc_shard_run* then continues with the unexpanded frontier.
    int shard_checkpoint(const char *path) override {
        if (!sh.ck_ok || sh.levels.empty()) { set_error("mc_shard_checkpoint: needs a sharded run that ended (finished, or stopped on a budget) without an error"); return MC_EBADCFG; }
        HIP_TRY(hipSetDevice(cfg.device));
        HIP_TRY(hipDeviceSynchronize());
        ShCkHeader h;
        memset(&h, 0, sizeof h);
        ck_fill_ident(h.id, CK_RANK);
        h.rank = cfg.shard_rank; h.world = nranks();
        h.table_cap = table_cap | (seen_sparse ? SEEN_SPARSE : 0); h.lo = sh.lo; h.hi = sh.hi; h.next = sh.next; h.dup = sh.dup; h.nlevels = sh.levels.size();
        DevCounters dc;
        HIP_TRY(hipMemcpy(&dc, d_ctr, sizeof dc, hipMemcpyDeviceToHost));
        ShCkCounters c;
        memset(&c, 0, sizeof c);
        c.arena_next = dc.arena_next; c.viol_key = dc.viol_key; c.via_list = dc.via_list; c.error = dc.error;
        for (int t = 0; t < NSHARD; t++) { c.generated[t] = dc.generated[t].v; c.cells[t] = dc.cells[t].v; }
        return ck_write(CK_RANK, path, {{&h, sizeof h}, {sh.levels.data(), sh.levels.size() * sizeof(uint64_t)}, {&c, sizeof c}}, ck_sections(sh.next, true));
    }
    int shard_restore_read(FILE *f, ShCkHeader &h, ShCkCounters &fc) {
        int rc = ck_read_header(CK_RANK, f, h);
        if (rc) return rc;
        const char *who = CK_RANK.reader;
        if (h.rank != cfg.shard_rank || h.world != nranks()) return ck_fail(MC_EBADCFG, who, "the file is another rank's, or of a run with another number of ranks");
        if (h.table_cap != (table_cap | (seen_sparse ? SEEN_SPARSE : 0)))
            return ck_fail(MC_EBADCFG, who, "table_capacity differs from the checkpointed run's, or the bucket form it implies (4 slots when the table is >= 3 x the arena): the seen-set slice is stored as it lay in HBM");
        if (h.next > arena_cap) return ck_fail(MC_EARENA, who, "arena_capacity is smaller than the checkpoint");
        if (h.lo > h.hi || h.hi != h.next || h.dup > h.next || h.nlevels == 0 || h.nlevels >= MC_MAX_LEVELS) return ck_fail(MC_EPARSE, who, "inconsistent header");
        if ((d_parent.p != nullptr) != (h.id.has_trace != 0)) return ck_fail(MC_EBADCFG, who, "MC_F_TRACE differs from the checkpointed run's");
        sh.levels.assign((size_t)h.nlevels, 0);
        if ((rc = ck_read_host(CK_RANK, f, {{sh.levels.data(), sh.levels.size() * sizeof(uint64_t)}, {&fc, sizeof fc}}))) return rc;
        if (fc.arena_next != h.next || fc.viol_key != ~0ull || fc.error) return ck_fail(MC_EPARSE, who, "inconsistent counters");
        HIP_TRY(hipSetDevice(cfg.device));
        HIP_TRY(hipDeviceSynchronize());
        if ((rc = ck_read_sections(f, ck_sections(h.next, true)))) return rc;
        if (fgetc(f) != EOF) return ck_fail(MC_EPARSE, who, "trailing bytes (not the file this engine's configuration wrote)");
        return MC_OK;
    }
    int shard_restore(const char *path) override {
        if (int rc = refuse_packed()) return rc;
        FileCloser f{fopen(path, "rb")};
        if (!f.f) return ck_fail(MC_EPARSE, "mc_shard_restore", std::string("cannot read ") + path);
        ShCkHeader h;
        ShCkCounters fc;
        if (int rc = shard_restore_read(f.f, h, fc)) { sh.levels.clear(); return rc; }
        DevCounters c;
        memset(&c, 0, sizeof c);
        c.arena_next = fc.arena_next; c.viol_key = fc.viol_key; c.via_list = fc.via_list;
        for (int t = 0; t < NSHARD; t++) { c.generated[t].v = fc.generated[t]; c.cells[t].v = fc.cells[t]; }
        HIP_TRY(hipMemcpy(d_ctr, &c, sizeof c, hipMemcpyHostToDevice));
        memset(kstat, 0, sizeof kstat);
        sh.lo = h.lo; sh.hi = h.hi; sh.next = h.next; sh.dup = h.dup;
        fr.last_distinct = sh.next;
        fr.have_viol = false;
        sh.sl[0].launched = sh.sl[1].launched = false;
        sh.resume = true;
        sh.ck_ok = false;
        return MC_OK;
    }

    int fetch_state(uint64_t idx, uint64_t *words) {
        const uint64_t *src = d_arena + ((idx >> 6) * (uint64_t)W) * 64 + (idx & 63);
        HIP_TRY(hipMemcpy2D(words, sizeof(uint64_t), src, 64 * sizeof(uint64_t), sizeof(uint64_t), W, hipMemcpyDeviceToHost));
        return MC_OK;
    }
    // arena indices from an initial state to the state the violation was found in / from
    int build_chain(std::vector<uint64_t> &chain) {
        chain.clear();
        if (!fr.have_viol) return MC_ESTATE;
        if (Viol(fr.last_viol).slot == SLOT_INIT) return MC_OK;  // violated by an initial state: handled by the caller
        return chain_to(viol_idx(fr.last_viol), chain);
    }
    int chain_to(uint64_t idx, std::vector<uint64_t> &chain) {   // ... to the stored state idx
        chain.clear();
        if (!d_parent) { set_error("engine created without MC_F_TRACE"); return MC_ESTATE; }
        for (int guard = 0; guard < MC_MAX_LEVELS; ++guard) {
            chain.push_back(idx);
            uint32_t p;
            HIP_TRY(hipMemcpy(&p, d_parent + idx, sizeof p, hipMemcpyDeviceToHost));
            if (p == 0xffffffffu) break;
            idx = p;
        }
        std::vector<uint64_t> rev(chain.rbegin(), chain.rend());
        chain.swap(rev);
        return MC_OK;
    }
    int trace(uint8_t *states_out, int32_t *actions_out, size_t *n_inout) override {
        if (sim.trace_n) return sim_trace_out(states_out, actions_out, n_inout);
        if (!fr.have_viol) { *n_inout = 0; return MC_OK; }
        HIP_TRY(hipSetDevice(cfg.device));
        const Viol v(fr.last_viol);
        if (v.slot == SLOT_INIT) {  // an initial state violates an invariant
            std::vector<uint64_t> words(W);
            S::init(prm, viol_idx(fr.last_viol), WordRef{words.data(), 1});
            std::vector<int32_t> acts{-1};
            return trace_out(words, acts, states_out, actions_out, n_inout);
        }
        return chain_trace(viol_idx(fr.last_viol), v.extra_state(), v.slot, states_out, actions_out, n_inout);
    }
    // the behaviour that ends in the stored state `end` (its parent chain), plus — extra — the successor rebuilt from (end, slot)
    int chain_trace(uint64_t end, bool extra, unsigned slot, uint8_t *states_out, int32_t *actions_out, size_t *n_inout) {
        std::vector<uint64_t> words, chain;
        std::vector<int32_t> acts;
        int rc = chain_to(end, chain);
        if (rc) return rc;
        words.resize(chain.size() * W);
        for (size_t k = 0; k < chain.size(); ++k) {
            if ((rc = fetch_state(chain[k], &words[k * W]))) return rc;
            if (k == 0) acts.push_back(-1);
            else {
                uint16_t ps;
                HIP_TRY(hipMemcpy(&ps, d_pslot + chain[k], sizeof ps, hipMemcpyDeviceToHost));
                acts.push_back(S::action_of(prm, &words[(k - 1) * W], (int)ps));
            }
        }
        if (extra) {  // append the violating successor
            std::vector<uint64_t> last(words.end() - W, words.end());
            words.resize(words.size() + W);
            S::apply(prm, CWordRef{last.data(), 1}, (int)slot, WordRef{&words[words.size() - W], 1});
            acts.push_back(S::action_of(prm, last.data(), (int)slot));
        }
        return trace_out(words, acts, states_out, actions_out, n_inout);
    }
    int trace_out(const std::vector<uint64_t> &words, const std::vector<int32_t> &acts, uint8_t *states_out, int32_t *actions_out, size_t *n_inout) {
        const size_t n = acts.size();
        if (n > *n_inout) { *n_inout = n; set_error("trace buffer too small"); return MC_EBADCFG; }
        if constexpr (HasExport<S>::value || RaftPacked<S>::value) {  // rows leave the engine in the spec's PUBLIC layout (generated code: the interpreter's row)
            for (size_t k = 0; k < n; ++k) S::export_row(prm, &words[k * W], (uint64_t *)states_out + k * export_words_of<S>(prm, W));
        } else
        memcpy(states_out, words.data(), n * W * sizeof(uint64_t));
        memcpy(actions_out, acts.data(), n * sizeof(int32_t));
        *n_inout = n;
        return MC_OK;
    }
    int read_states(uint64_t first, uint64_t count, uint8_t *out) override {
        if (!count) return MC_OK;
        if (first + count > fr.last_distinct) { set_error("read_states: range beyond the states found by the last run"); return MC_EBADCFG; }
        HIP_TRY(hipSetDevice(cfg.device));
        DevBuf<uint64_t> tmp;
        const uint64_t piece = 1ull << 20;
        HIP_TRY(tmp.alloc((count < piece ? count : piece) * W));
        for (uint64_t off = 0; off < count; off += piece) {
            const uint64_t n = count - off < piece ? count - off : piece;
            hipLaunchKernelGGL(k_gather_states, dim3((unsigned)((n * W + 255) / 256)), dim3(256), 0, stream, d_arena, W, first + off, n, tmp);
            hipError_t e1, e2;
            if constexpr (HasExport<S>::value || RaftPacked<S>::value) {
                std::vector<uint64_t> rows((size_t)n * W);
                e1 = hipMemcpyAsync(rows.data(), tmp, n * W * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
                e2 = hipStreamSynchronize(stream);
                if (e1 == hipSuccess && e2 == hipSuccess)
                    for (uint64_t k = 0; k < n; ++k) S::export_row(prm, &rows[(size_t)k * W], (uint64_t *)out + (size_t)(off + k) * export_words_of<S>(prm, W));
            } else {
                e1 = hipMemcpyAsync(out + off * W * sizeof(uint64_t), tmp, n * W * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
                e2 = hipStreamSynchronize(stream);
            }
            if (e1 != hipSuccess || e2 != hipSuccess) { set_error("read_states: copy failed"); return MC_EHIP; }
        }
        return MC_OK;
    }
    // Profiling aid: expand every resident state again (seen-set already full, so every probe hits)
    // with optional ablation flags; returns the kernel time.  State counts are not changed.
    int debug_flags(uint32_t set, uint32_t clear) override { cfg.flags = (cfg.flags & ~clear) | set; return MC_OK; }
    int seen_layout(uint64_t *buckets, uint32_t *slots) override {
        *buckets = seen_arg() & ~SEEN_SPARSE;
        *slots = seen_sparse ? MC_SPARSE_SLOTS : 8;
        return MC_OK;
    }
    int debug_phases(uint64_t *out48, int reset) override {
#ifdef MC_PHASE_PROF
        HIP_TRY(hipSetDevice(cfg.device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpyFromSymbol(out48, HIP_SYMBOL(g_phase), 48 * sizeof(uint64_t)));
        if (reset) { static const unsigned long long zero[48] = {}; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_phase), zero, sizeof zero)); }
        return MC_OK;
#else
        (void)out48; (void)reset;
        set_error("the library was built without MC_PHASE_PROF");
        return MC_ESTATE;
#endif
    }
    int debug_reexpand(unsigned extra_flags, double *ms) override {
        HIP_TRY(hipSetDevice(cfg.device));
        Event a(hipEventDefault), b(hipEventDefault);  // (timing events)
        HIP_TRY(hipEventRecord(a.get(), stream));
        for (uint64_t c0 = 0; c0 < fr.last_distinct; c0 += chunk) {
            const uint64_t c1 = c0 + chunk < fr.last_distinct ? c0 + chunk : fr.last_distinct;
            const uint64_t ncols = ((c1 - c0) + 63) & ~63ull;
            launch_expand<S, false>(!((cfg.flags | extra_flags) & MC_F_NOFAMILY), cfg.flags | extra_flags, ncols, stream, 0u, prm,
                                    (const uint64_t *)d_arena, c0, c1, ncols, d_table.p, seen_arg(), d_newlist.p, seg_cap, d_ctr.p,
                                    cfg.flags | extra_flags, RouteArgs{}, 0u);
            hipLaunchKernelGGL(k_commit, dim3(1), dim3(1), 0, stream, d_ctr, 0u);
        }
        HIP_TRY(hipEventRecord(b.get(), stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, a.get(), b.get()));
        *ms = t;
        // restore arena_next (k_commit added nothing: no probe can be new) and leave counters as they were
        return MC_OK;
    }
    // ------------------------------------------------------------------ sharded step API
    // the slot's exchange buffers for rounds of up to send_cap candidates (grow-only; every caller of a slot passes through here)
    int shard_alloc(ShSlot &q, uint64_t send_cap) {
        const unsigned P = nranks();
        if (send_cap > q.pend_src.n) {  // all three go before any comes back, pend_src last: its size is the capacity the slot answers for
            q.rt_fp.reset(); q.rt_src.reset(); q.pend_src.reset();
            q.rt_subcap = (send_cap / (P * NSHARD)) * 2 + 4096;
            HIP_TRY(q.rt_fp.alloc((size_t)P * NSHARD * q.rt_subcap));
            HIP_TRY(q.rt_src.alloc((size_t)P * NSHARD * q.rt_subcap));
            HIP_TRY(q.pend_src.alloc(send_cap));
        }
        HIP_TRY(q.rt_cur.reserve((size_t)(P * NSHARD)));
        if (send_cap > sh.d_incl.n) {
            sh.d_new_src.reset(); sh.d_incl.reset();
            HIP_TRY(sh.d_new_src.alloc(send_cap));
            HIP_TRY(sh.d_incl.alloc(send_cap));
        }
        HIP_TRY(sh.d_ends.reserve(8));
        HIP_TRY(sh.h_ends.reserve(8));
        HIP_TRY(sh.h_cur.reserve((size_t)8 * NSHARD));
        return MC_OK;
    }
    // generated code with packed rows serves one GPU: its rows cannot travel between ranks
    static int refuse_packed() {
        if constexpr (PackedRows<S>::value) { set_error("this engine of generated code stores rows packed to its program's cell ranges and serves ONE GPU: create a sharded engine with shard_count > 1 (or $TLAMC_JIT_PACK=0)"); return MC_EBADCFG; }
        // (a raft engine that has not searched yet never gets here: the mc_shard_* entries re-create it with the rows the step calls exchange)
        if constexpr (RaftPacked<S>::value) { set_error("this raft engine has searched with its rows stored in fewer words (one GPU) and cannot go on in sharded steps: create the engine with shard_count > 1, make the mc_shard_* call before the first search, or set $TLAMC_RAFT_PACK=0"); return MC_EBADCFG; }
        return MC_OK;
    }
    // 0: the engine stores the rows the C ABI hands out; 1: narrower ones, and nothing has been searched, restored or simulated yet; 2: narrower ones, in use
    int narrow_rows() const override {
        if constexpr (!RaftPacked<S>::value) return 0;
        return !fr.have_run && !ck.pending && !sim.trace_n && fr.last_distinct == 0 ? 1 : 2;
    }
    // a sharded run that failed mid-level (a full route bucket, MC_ETABLEFULL ...) leaves its slots as they were: the remedy the
    // error message names — run the same engine again with a larger allowance — must not trip over an expand "still in flight"
    void shard_reset_slots() {
        hipSetDevice(cfg.device);
        hipDeviceSynchronize();  // (whatever the failed run left on the streams has drained; its events are complete)
        for (auto &q : sh.sl) { q.launched = false; q.keep_pending = false; q.pend_total = 0; q.moved = 0; q.count = 0; }
    }
    int shard_begin() override {
        int rc = refuse_packed();
        if (rc) return rc;
        if (nranks() > 8) { set_error("at most 8 shards"); return MC_EBADCFG; }
        sh.dup = 0;
        sh.resume = sh.ck_ok = false;
        shard_reset_slots();
        HIP_TRY(hipSetDevice(cfg.device));
        memset(kstat, 0, sizeof kstat);
        if ((rc = seed_init(cfg.shard_rank, cfg.shard_count, false, false, nullptr))) return rc;
        if ((rc = read_counters())) return rc;
        if ((rc = check_dev_error())) return rc;
        sh.lo = 0;
        sh.hi = sh.next = h_ctr->arena_next;
        fr.last_distinct = sh.next;
        return MC_OK;
    }
    // The first levels of a run are tiny: sharding them costs several collectives per level and balances nothing.
    // Every rank therefore runs the SAME fused BFS (run()) until a level has at least min_frontier states, keeps every
    // nranks-th state of that level as its local frontier, and the sharded rounds start there.  The seen-set of each
    // rank then holds ALL prefix fingerprints (a superset of the ones it owns: harmless); rank 0 alone reports the
    // prefix's `generated`, and distinct_local excludes what other ranks already count.
    int shard_begin_replicated(uint64_t min_frontier, uint64_t max_distinct, uint64_t max_levels, uint64_t *levels_out, uint32_t *nlevels) override {
        if (int rc = refuse_packed()) return rc;
        if (nranks() > 8) { set_error("at most 8 shards"); return MC_EBADCFG; }
        mc_result &res = *sh.prefix_res;  // (not shared between engines / threads)
        sh.resume = sh.ck_ok = false;
        shard_reset_slots();
        const uint64_t saved_md = cfg.max_distinct, saved_ml = cfg.max_levels;
        cfg.max_distinct = max_distinct;  // the whole job's budgets: the prefix stops where the single-GPU run would
        cfg.max_levels = max_levels;
        fr.stop_frontier = min_frontier ? min_frontier : 1;
        const int rc = run(&res);
        fr.stop_frontier = 0;
        cfg.max_distinct = saved_md;
        cfg.max_levels = saved_ml;
        if (rc) return rc;
        const uint32_t cap = *nlevels;
        *nlevels = res.levels;
        for (uint32_t k = 0; k < res.levels && k < cap; k++) levels_out[k] = res.level_distinct[k];
        if (res.levels > cap) { set_error("shard_begin_replicated: level buffer too small"); return MC_EBADCFG; }
        const unsigned P = nranks(), r = cfg.shard_rank;
        const uint64_t lo = fr.lo, hi = fr.hi;
        const bool go_on = h_ctr->viol_key == ~0ull && hi > lo;  // otherwise finished or failed inside the prefix
        if (go_on)
            hipLaunchKernelGGL(k_take_owned<S>, dim3((unsigned)((hi - lo + 255) / 256)), dim3(256), 0, stream, prm, d_arena, lo, hi, r, P, hi,
                               arena_cap, d_parent, d_pslot, d_ctr);
        hipLaunchKernelGGL(k_after_prefix, dim3(1), dim3(1), 0, stream, d_ctr, (unsigned long long)hi, r != 0 ? 1 : 0);
        int rc2 = read_counters();
        if (rc2) return rc2;
        if ((rc2 = check_dev_error())) return rc2;
        sh.lo = hi;
        sh.hi = sh.next = h_ctr->arena_next;
        sh.dup = r == 0 ? sh.hi - hi : sh.hi;
        fr.last_distinct = sh.next;
        return MC_OK;
    }
    int shard_level_size(uint64_t *n) override { *n = sh.hi - sh.lo; return MC_OK; }
    int shard_note_levels(const uint64_t *levels, uint32_t n, int32_t verdict) override {
        sh.levels.assign(levels, levels + n);
        sh.ck_ok = verdict == MC_V_OK || verdict == MC_V_BUDGET;
        return MC_OK;
    }
    int shard_resume(uint64_t *levels_out, uint32_t *nlevels) override {
        const uint32_t cap = *nlevels;
        *nlevels = 0;
        if (!sh.resume) return MC_OK;
        if (sh.levels.size() > cap) { set_error("shard_resume: level buffer too small"); return MC_EBADCFG; }
        for (size_t k = 0; k < sh.levels.size(); k++) levels_out[k] = sh.levels[k];
        *nlevels = (uint32_t)sh.levels.size();
        sh.resume = false;
        return MC_OK;
    }
    int shard_info(void **main_stream, uint64_t *chunk_states, int32_t *traced) override {
        HIP_TRY(hipSetDevice(cfg.device));
        if (main_stream) *main_stream = (void *)stream;
        if (chunk_states) *chunk_states = chunk;
        if (traced) *traced = d_parent.p != nullptr;
        return MC_OK;
    }
    size_t state_bytes() const override { return (size_t)W * 8; }
    // the side stream of the sharded path (Shard::sh.ext_stream)
    hipStream_t side() const { return sh.ext_side ? sh.ext_stream : stream2; }
    void append_begin(hipStream_t s) { if (sh.ev_append.made()) hipStreamWaitEvent(s, sh.ev_append.get(), 0); }  // (Shard::sh.ev_append)
    void append_end(hipStream_t s) { hipEventRecord(sh.ev_append.get(), s); }
    int side_done() {
        if (!sh.ext_side) HIP_TRY(hipStreamSynchronize(stream2));
        return MC_OK;
    }
    int shard_set_stream(void *hip_stream, int enable) override {
        HIP_TRY(hipSetDevice(cfg.device));
        HIP_TRY(hipStreamSynchronize(side()));
        sh.ext_stream = (hipStream_t)hip_stream;
        sh.ext_side = enable != 0;
        return MC_OK;
    }
    // The locally owned new states of the slot's chunk (local-owner shortcut; new-list parity = slot): materialised on the second
    // stream, in order with the other kernels that append at arena_next (keep, ingest).  The caller has ordered stream2 behind the expand.
    int materialise_local(unsigned slot) {
        const ShSlot &q = sh.sl[slot];
        append_begin(stream2);
        timed(2, 0, [&] {
            hipLaunchKernelGGL(k_materialise<S>, dim3(mat_grid(q.ncols), NSHARD), dim3(256), 0, stream2, prm, d_arena, q.chunk_base, d_newlist, seg_cap,
                               arena_cap, d_parent, d_pslot, d_ctr, slot, (const LevelCtl *)nullptr, (const uint64_t *)d_newfp);
        }, stream2);
        hipLaunchKernelGGL(k_commit, dim3(1), dim3(1), 0, stream2, d_ctr, slot);
        append_end(stream2);
        HIP_TRY(hipEventRecord(sh.ev_mat[slot].get(), stream2));
        return MC_OK;
    }
    int shard_expand_launch(unsigned slot, uint64_t first, uint64_t count, uint64_t send_cap) override {
        HIP_TRY(hipSetDevice(cfg.device));
        if (slot > 1) { set_error("shard_expand: slot must be 0 or 1"); return MC_EBADCFG; }
        ShSlot &q = sh.sl[slot];
        const unsigned P = nranks();
        int rc = shard_alloc(q, send_cap);
        if (rc) return rc;
        q.pend_total = 0;
        q.count = count;
        q.launched = true;
        for (unsigned t = 0; t <= 8; t++) q.pend_off.off[t] = 0;
        if (first + count > sh.hi - sh.lo) { set_error("shard_expand: chunk outside the local frontier"); return MC_EBADCFG; }
        if (count > chunk) { set_error("shard_expand: chunk larger than chunk_states"); return MC_EBADCFG; }
        if (!count) return MC_OK;
        if (sh.ev_slot[slot].made()) HIP_TRY(hipStreamWaitEvent(stream, sh.ev_slot[slot].get(), 0));  // the slot's previous buckets have been compacted
        if (sh.ev_mat[slot].made()) HIP_TRY(hipStreamWaitEvent(stream, sh.ev_mat[slot].get(), 0));  // ... and its locally owned new states written
        HIP_TRY(hipMemsetAsync(q.rt_cur, 0, (size_t)(P * NSHARD) * sizeof(PaddedCounter), stream));
        const uint64_t c0 = sh.lo + first, c1 = c0 + count, base = c0 & ~63ull;
        const uint64_t ncols = ((c1 - base) + 63) & ~63ull;
        q.chunk_base = base;
        RouteArgs rt{P, q.rt_cur, q.rt_fp, q.rt_src, q.rt_subcap};
        rt.my_rank = cfg.shard_rank;
        rt.new_fp = d_newfp;
        q.ncols = ncols;
        timed(0, count, [&] {  // new-list parity = slot: the locally owned new states of this chunk (local-owner shortcut)
            launch_expand<S, true>(!(cfg.flags & MC_F_NOFAMILY), cfg.flags, ncols, stream, 0u, prm,
                                   (const uint64_t *)d_arena, c0, c1, ncols, d_table.p, seen_arg(), d_newlist.p, seg_cap, d_ctr.p, cfg.flags, rt, slot);
        });
        return MC_OK;
    }
    int shard_expand_finish(unsigned slot, uint64_t *send_fp, uint64_t send_cap, uint64_t *send_counts) override {
        HIP_TRY(hipSetDevice(cfg.device));
        if (slot > 1 || !sh.sl[slot].launched) { set_error("shard_expand_finish: no expand in flight for this slot"); return MC_EBADCFG; }
        ShSlot &q = sh.sl[slot];
        q.launched = false;
        const unsigned P = nranks();
        for (unsigned t = 0; t < P; t++) send_counts[t] = 0;
        if (!q.count) return MC_OK;
        // one wait on the expand stream only: the side stream may still be busy with the previous round
        PaddedCounter *cur = sh.h_cur;
        HIP_TRY(hipMemcpyAsync(cur, q.rt_cur, (size_t)(P * NSHARD) * sizeof(PaddedCounter), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(h_ctr, d_ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        int rc;
        if ((rc = check_dev_error())) return rc;
        uint64_t total = 0;
        for (unsigned t = 0; t < P; t++) {
            q.pend_off.off[t] = total;
            for (unsigned x = 0; x < NSHARD; x++) {
                if (cur[t * NSHARD + x].v > q.rt_subcap) { set_error("shard_expand: route bucket overflow (raise send_cap)"); return MC_EROUTE; }
                send_counts[t] += cur[t * NSHARD + x].v;
            }
            total += send_counts[t];
        }
        for (unsigned t = P; t <= 8; t++) q.pend_off.off[t] = total;
        // (the pending list is as long as the largest send capacity asked for so far: more candidates than it holds is "more successors
        //  per state than the fan-out allowance" — MC_EROUTE, the level loop starts over with twice the allowance — not a full arena)
        if (total >= (1ull << 31)) { set_error("shard_expand: more than 2^31 candidates in one round (lower chunk_states)"); return MC_EARENA; }
        if (total > q.pend_src.n) { set_error("shard_expand: more candidates in one round than the slot's pending list holds (raise the fan-out allowance)"); return MC_EROUTE; }
        if (total > send_cap) { set_error("shard_expand: send buffer too small (raise the fan-out allowance)"); return MC_EROUTE; }
        q.pend_total = total;
        if (q.keep_pending) {  // the slot's previous keep still reads pend_src
            HIP_TRY(hipStreamWaitEvent(side(), sh.ev_keep[slot].get(), 0));
            q.keep_pending = false;
        }
        if ((rc = materialise_local(slot))) return rc;  // (the expand kernel has finished: stream was synchronised)
        if (total) {
            RouteArgs rt{P, q.rt_cur, q.rt_fp, q.rt_src, q.rt_subcap};
            hipLaunchKernelGGL(k_compact_buckets, dim3(64, P * NSHARD), dim3(256), 0, side(), rt, send_fp, q.pend_src);
        }
        HIP_TRY(hipEventRecord(sh.ev_slot[slot].get(), side()));
        return side_done();
    }
    int shard_probe(const uint64_t *recv_fp, uint64_t n, uint8_t *answers) override {
        HIP_TRY(hipSetDevice(cfg.device));
        if (!n) return MC_OK;
        timed(1, n, [&] {
            hipLaunchKernelGGL(k_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, side(), recv_fp, n, d_table, seen_arg(), answers, d_ctr);
        }, side());
        return side_done();
    }
    // ---- fixed-capacity rounds: nothing of a round waits for the host (sizes travel in band; errors surface at shard_end_level)
    int shard_expand_pack(unsigned slot, uint64_t *send_fp, uint64_t cap) override {
        HIP_TRY(hipSetDevice(cfg.device));
        if (slot > 1 || !sh.sl[slot].launched) { set_error("shard_expand_pack: no expand in flight for this slot"); return MC_EBADCFG; }
        ShSlot &q = sh.sl[slot];
        q.launched = false;
        const unsigned P = nranks();
        if (cap < 2 || (uint64_t)P * cap > q.pend_src.n || (uint64_t)P * cap >= (1ull << 31)) { set_error("shard_expand_pack: capacity does not fit the slot's buffers"); return MC_EBADCFG; }
        q.pend_total = (uint64_t)P * cap;  // the sender scans the whole packed range: answers outside the counts are 0
        for (unsigned t = 0; t <= 8; t++) q.pend_off.off[t] = (t < P ? t : P) * cap;
        HIP_TRY(hipEventRecord(sh.ev_exp[slot].get(), stream));  // behind the slot's expand kernel (or behind nothing: an empty chunk)
        // The buckets are compacted on the EXPAND stream, right behind the kernel that filled them: on the side stream the
        // compaction of round r+1 would queue behind the probes of round r (or those behind it), and the fingerprint exchange of
        // round r+1 could never overlap them.  The caller orders its collective behind this call with an event on that stream
        // (mc_shard_info hands it out).
        if (q.keep_pending) {  // the slot's previous keep still reads pend_src
            HIP_TRY(hipStreamWaitEvent(stream, sh.ev_keep[slot].get(), 0));
            q.keep_pending = false;
        }
        if (q.count) {  // the chunk's locally owned new states (local-owner shortcut), as in shard_expand_finish
            HIP_TRY(hipStreamWaitEvent(stream2, sh.ev_exp[slot].get(), 0));
            const int rc = materialise_local(slot);
            if (rc) return rc;
            RouteArgs rt{P, q.rt_cur, q.rt_fp, q.rt_src, q.rt_subcap};
            hipLaunchKernelGGL(k_compact_packed, dim3(64, P * NSHARD), dim3(256), 0, stream, rt, cap, send_fp, q.pend_src, d_ctr);
        } else {  // no chunk for this rank in this round: empty buckets
            for (unsigned t = 0; t < P; t++) HIP_TRY(hipMemsetAsync(send_fp + (uint64_t)t * cap, 0, sizeof(uint64_t), stream));
        }
        HIP_TRY(hipEventRecord(sh.ev_slot[slot].get(), stream));
        if (!sh.ext_side) HIP_TRY(hipStreamSynchronize(stream));
        return side_done();
    }
    int shard_probe_pack(const uint64_t *recv_fp, uint64_t cap, uint8_t *answers) override {
        HIP_TRY(hipSetDevice(cfg.device));
        const uint64_t total = (uint64_t)nranks() * cap;
        if (!total) return MC_OK;
        timed(1, total, [&] {
            hipLaunchKernelGGL(k_probe_packed, dim3((unsigned)(nranks() * ((cap + 255) / 256))), dim3(256), 0, side(), recv_fp, cap, nranks(), d_table,
                               seen_arg(), answers, d_ctr);
        }, side());
        return side_done();
    }
    int shard_keep_pack(unsigned slot, const uint8_t *answers_back, uint64_t cap) override {
        if (slot > 1 || sh.sl[slot].pend_total != (uint64_t)nranks() * cap) { set_error("shard_keep_pack: not the capacity the slot was packed with"); return MC_EBADCFG; }
        return shard_keep(slot, answers_back, nullptr);
    }
    // the caller's stream waits (on the device) until the slot's last keep has consumed its answers buffer: a caller that
    // reuses ONE answers buffer per slot calls this before the collective that overwrites it
    int shard_wait_keep(unsigned slot) override {
        if (slot > 1) return MC_EBADCFG;
        HIP_TRY(hipSetDevice(cfg.device));
        if (sh.sl[slot].keep_pending) HIP_TRY(hipStreamWaitEvent(side(), sh.ev_keep[slot].get(), 0));  // (pending: the event has been recorded)
        return MC_OK;
    }
    int shard_materialise(unsigned slot, const uint8_t *answers_back, uint8_t *send_states, uint64_t send_cap, uint64_t *send_counts) override {
        HIP_TRY(hipSetDevice(cfg.device));
        if (slot > 1) return MC_EBADCFG;
        ShSlot &q = sh.sl[slot];
        const unsigned P = nranks();
        for (unsigned t = 0; t < P; t++) send_counts[t] = 0;
        q.moved = 0;
        if (!q.pend_total) return MC_OK;
        const unsigned bx = (unsigned)((q.pend_total + 255) / 256);
        int rc = scan_answers_inclusive(answers_back, sh.d_incl.p, q.pend_total, sh.d_scan_tmp, side());
        if (rc) return rc;
        hipLaunchKernelGGL(k_gather_range_ends, dim3(1), dim3(64), 0, side(), sh.d_incl, q.pend_off, P, sh.d_ends);
        unsigned long long *ends = sh.h_ends;  // the per-owner counts go back to the host: the caller sizes its all-to-all with them
        HIP_TRY(hipMemcpyAsync(ends, sh.d_ends, P * sizeof(unsigned long long), hipMemcpyDeviceToHost, side()));
        HIP_TRY(hipStreamSynchronize(side()));
        OwnerOffsets start;
        std::vector<PaddedCounter> cnt(P);
        for (unsigned t = 0; t <= 8; t++) start.off[t] = 0;
        for (unsigned t = 0; t < P; t++) {
            start.off[t] = t ? ends[t - 1] : 0;
            cnt[t].v = ends[t] - start.off[t];
        }
        hipLaunchKernelGGL(k_compact_new, dim3(bx), dim3(256), 0, side(), answers_back, sh.d_incl, q.pend_src, q.pend_total, q.pend_off, start, P,
                           sh.d_new_src);
        BlockPlan plan;
        uint64_t blocks = 0;
        for (unsigned t = 0; t < 8; t++) {
            plan.blk_off[t] = blocks;
            plan.cnt[t] = t < P ? cnt[t].v : 0;
            if (t < P) { send_counts[t] = cnt[t].v; blocks += (cnt[t].v + 63) / 64; }
        }
        plan.blk_off[8] = blocks;
        for (unsigned t = P; t < 8; t++) plan.blk_off[t] = blocks;
        q.plan = plan;
        q.moved = 0;
        for (unsigned t = 0; t < P; t++) q.moved += plan.cnt[t];
        if (blocks * 64 > send_cap) { set_error("shard_materialise: state send buffer too small"); return MC_EARENA; }  // (the loop sizes it for the upper bound and repeats)
        if (blocks) {
            timed(2, blocks * 64, [&] {
                hipLaunchKernelGGL(k_send_materialise<S>, dim3((unsigned)((blocks * 64 + 255) / 256)), dim3(256), 0, side(), prm, d_arena,
                                   q.chunk_base, sh.d_new_src, q.pend_off, plan, P, (uint64_t *)send_states);
            }, side());
        }
        return side_done();
    }
    // "stay" mode: materialise the positively answered candidates of slot's expand into the LOCAL arena.
    // The count of new states stays on the device (arena_next); the host learns it at shard_end_level.
    int shard_keep(unsigned slot, const uint8_t *answers_back, uint64_t *n_new) override {
        HIP_TRY(hipSetDevice(cfg.device));
        if (n_new) *n_new = 0;
        if (slot > 1) return MC_EBADCFG;
        ShSlot &q = sh.sl[slot];
        if (!q.pend_total) return MC_OK;
        const unsigned bx = (unsigned)((q.pend_total + 255) / 256);
        // keep runs on the engine's own second stream, behind the caller's stream at this point (the answers
        // are ready there), so the caller's next exchange does not queue behind the materialisation
        hipStream_t ks = stream2;
        if (sh.ext_side) {
            HIP_TRY(hipEventRecord(sh.ev_ans.get(), sh.ext_stream));
            HIP_TRY(hipStreamWaitEvent(ks, sh.ev_ans.get(), 0));
        }
        int rc = scan_answers_inclusive(answers_back, sh.d_incl.p, q.pend_total, sh.d_scan_tmp, ks);
        if (rc) return rc;
        append_begin(ks);
        const uint32_t *d_total = sh.d_incl + (q.pend_total - 1);
        OwnerOffsets one, zero;  // a single range covering every pending candidate
        for (unsigned t = 0; t <= 8; t++) { one.off[t] = t ? q.pend_total : 0; zero.off[t] = 0; }
        hipLaunchKernelGGL(k_compact_new, dim3(bx), dim3(256), 0, ks, answers_back, sh.d_incl, q.pend_src, q.pend_total, one, zero, 1u, sh.d_new_src);
        // grid sized for the upper bound (every candidate new); surplus threads leave at once
        timed(2, 0, [&] {
            hipLaunchKernelGGL(k_materialise_list<S>, dim3(bx), dim3(256), 0, ks, prm, d_arena, q.chunk_base, sh.d_new_src, d_total, arena_cap,
                               d_parent, d_pslot, d_ctr);
        }, ks);
        hipLaunchKernelGGL(k_bump_arena_next, dim3(1), dim3(1), 0, ks, d_ctr, d_total, 0ull, (unsigned long long)arena_cap);
        append_end(ks);
        HIP_TRY(hipEventRecord(sh.ev_keep[slot].get(), ks));
        q.keep_pending = true;
        if (!sh.ext_side) {
            uint32_t total32 = 0;
            HIP_TRY(hipMemcpyAsync(&total32, d_total, sizeof total32, hipMemcpyDeviceToHost, ks));
            HIP_TRY(hipStreamSynchronize(ks));
            if (n_new) *n_new = total32;
        }
        return MC_OK;
    }
    // recv_states: one bucket per source rank, back to back, each a whole number of 64-state blocks;
    // n = valid states of ONE bucket starting at recv_states (call once per source)
    int shard_ingest(const uint8_t *recv_states, uint64_t n) override {
        HIP_TRY(hipSetDevice(cfg.device));
        if (!n) return MC_OK;
        append_begin(side());
        hipLaunchKernelGGL(k_ingest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, side(), d_arena, W, (const uint64_t *)recv_states, n,
                           arena_cap, d_parent, d_ctr);
        hipLaunchKernelGGL(k_bump_arena_next, dim3(1), dim3(1), 0, side(), d_ctr, (const uint32_t *)nullptr, (unsigned long long)n,
                           (unsigned long long)arena_cap);
        append_end(side());
        return side_done();
    }
    // (parent index on this rank << 16 | slot) of the states the slot's last shard_materialise put into its send buffer, same
    // order (owner by owner, without the block padding); call it before the next shard_materialise / shard_keep of any slot
    int shard_materialise_parents(unsigned slot, uint64_t *send_parents) override {
        HIP_TRY(hipSetDevice(cfg.device));
        if (slot > 1) return MC_EBADCFG;
        ShSlot &q = sh.sl[slot];
        if (!q.moved) return MC_OK;
        hipLaunchKernelGGL(k_send_parents, dim3((unsigned)((q.moved + 255) / 256)), dim3(256), 0, side(), (const uint32_t *)sh.d_new_src, q.chunk_base,
                           q.pend_off, q.plan, nranks(), send_parents);
        return side_done();
    }
    // right after the shard_ingest of the same bucket: the n states just appended came from `src_rank`
    int shard_ingest_parents(const uint64_t *recv_parents, uint64_t n, unsigned src_rank) override {
        HIP_TRY(hipSetDevice(cfg.device));
        if (!n || !d_prank) return MC_OK;  // without MC_F_TRACE nothing is recorded
        hipLaunchKernelGGL(k_ingest_parents, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, side(), recv_parents, n, src_rank, d_parent, d_pslot,
                           d_prank, (const DevCounters *)d_ctr);
        return side_done();
    }
    int shard_violation(int32_t *found, uint64_t *idx, uint32_t *slot, int32_t *verdict, int32_t *invariant) override {
        HIP_TRY(hipSetDevice(cfg.device));
        HIP_TRY(hipStreamSynchronize(side()));
        int rc = read_counters();
        if (rc) return rc;
        *found = h_ctr->viol_key != ~0ull;
        *idx = 0; *slot = 0; *verdict = MC_V_OK; *invariant = -1;
        if (*found) {
            const Viol v(h_ctr->viol_key);
            *idx = viol_idx(h_ctr->viol_key);
            *slot = v.slot;
            *verdict = v.verdict;
            *invariant = v.invariant;
        }
        return MC_OK;
    }
    // one step of a counterexample walk: the state at arena index idx of THIS rank and where its parent lives
    // (parent_rank == shard_rank: here; parent_idx == 0xffffffff: an initial state; parent_slot 0xfffc: the entry is a copy
    // of state parent_idx made by the replicated prefix, not a step)
    int shard_fetch(uint64_t idx, uint8_t *state_out, uint32_t *parent_rank, uint64_t *parent_idx, uint32_t *parent_slot) override {
        HIP_TRY(hipSetDevice(cfg.device));
        if (idx & (1ull << 63)) {  // an initial state, rebuilt from its ordinal in Init's enumeration (a violating initial state is not looked up in the arena)
            const uint64_t ord = idx & ~(1ull << 63);
            if (ord >= S::num_init(prm)) return MC_EBADCFG;
            S::init(prm, ord, WordRef{(uint64_t *)state_out, 1});
            *parent_rank = cfg.shard_rank;
            *parent_idx = 0xffffffffull;
            *parent_slot = SLOT_INIT;
            return MC_OK;
        }
        if (!d_parent) { set_error("engine created without MC_F_TRACE"); return MC_ESTATE; }
        if (idx >= arena_cap) return MC_EBADCFG;
        HIP_TRY(hipDeviceSynchronize());
        int rc = fetch_state(idx, (uint64_t *)state_out);
        if (rc) return rc;
        uint32_t p = 0;
        uint16_t ps = 0;
        uint8_t pr = 0xff;
        HIP_TRY(hipMemcpy(&p, d_parent + idx, sizeof p, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&ps, d_pslot + idx, sizeof ps, hipMemcpyDeviceToHost));
        if (d_prank) HIP_TRY(hipMemcpy(&pr, d_prank + idx, sizeof pr, hipMemcpyDeviceToHost));
        *parent_rank = pr == 0xff ? cfg.shard_rank : pr;
        *parent_idx = p;
        *parent_slot = ps;
        return MC_OK;
    }
    int shard_end_level(uint64_t *new_local) override {
        HIP_TRY(hipSetDevice(cfg.device));
        if (sh.sl[0].launched || sh.sl[1].launched) { set_error("shard_end_level: an expand is still in flight"); return MC_EBADCFG; }
        HIP_TRY(hipStreamSynchronize(side()));
        HIP_TRY(hipStreamSynchronize(stream2));
        int rc = read_counters();
        if (rc) return rc;
        if ((rc = check_dev_error())) return rc;
        sh.next = h_ctr->arena_next;
        fr.last_distinct = sh.next;
        sh.lo = sh.hi;
        sh.hi = sh.next;
        *new_local = sh.hi - sh.lo;
        return MC_OK;
    }
    // invariants of the unexpanded frontier [lo, hi) for specs that check on expansion (see k_check_frontier); no-op otherwise
    int check_frontier(uint64_t lo, uint64_t hi) {
        if constexpr (ChecksOnExpand<S>::value) {
            if (hi > lo) {
                hipLaunchKernelGGL(k_check_frontier<S>, dim3((unsigned)((hi - lo + 255) / 256)), dim3(256), 0, stream, prm,
                                   (const uint64_t *)d_arena, lo, hi, d_ctr);
                return read_counters();
            }
        }
        return MC_OK;
    }
    int shard_check_frontier() override {
        HIP_TRY(hipSetDevice(cfg.device));
        HIP_TRY(hipStreamSynchronize(side()));
        HIP_TRY(hipStreamSynchronize(stream2));
        return check_frontier(sh.lo, sh.hi);
    }
    int shard_counters(uint64_t *generated, uint64_t *distinct_local, int32_t *verdict) override {
        HIP_TRY(hipSetDevice(cfg.device));
        HIP_TRY(hipStreamSynchronize(side()));
        int rc = read_counters();
        if (rc) return rc;
        if ((rc = check_dev_error())) return rc;
        *generated = 0;
        for (int t = 0; t < NSHARD; t++) *generated += h_ctr->generated[t].v;
        *distinct_local = h_ctr->arena_next - sh.dup;
        *verdict = h_ctr->viol_key != ~0ull ? Viol(h_ctr->viol_key).verdict : MC_V_OK;
        return MC_OK;
    }
    // ------------------------------------------------------------------------------- simulation (mc_engine_simulate; engine_sim.h)
    // Walks run in rounds of SIM_ROUND (fixed: a run's result must not depend on the device), each round in launches of SIM_ITERS
    // walk events; the host reads the counters between launches (stop requests, progress, the end of a round).  The walk buffers are
    // allocated on first use and live until the engine is destroyed; they are not the BFS's arena.
    static constexpr uint64_t SIM_ROUND = 1ull << 18;
    static constexpr uint32_t SIM_ITERS = 16;
    static constexpr uint64_t SIM_MAX_WALKS = 1ull << 40;   // walk indices of a run (the walk field of a violation key, sim_walk.h)
    // one round: walks w0 .. w0+n-1 from their start to their end (or to a stop request); the counters accumulate in sim.ctr.
    // *complete: every walk of the round ended.  Progress is reported (and a stop request seen) after EVERY launch, the round's last
    // one included: a model whose walks all end within one launch must not run an unbounded simulation past mc_engine_request_stop.
    int sim_round(SimArgs a, uint64_t n, SimCounters &c, uint64_t walks_before, bool allow_stop, uint64_t rounds_done, bool *complete) {
        a.n = n;
        a.ncols = (n + 63) & ~63ull;
        *complete = false;
        HIP_TRY(hipMemsetAsync(sim.wst, 0, n * sizeof(uint32_t), stream));
        const unsigned blocks = (unsigned)((a.ncols + 255) / 256);
        const uint64_t launches = ((uint64_t)a.depth + 1 + SIM_ITERS - 1) / SIM_ITERS;  // depth + 1 events end every walk
        for (uint64_t l = 0; l < launches; ++l) {
            hipLaunchKernelGGL(k_simulate<S>, dim3(blocks), dim3(256), 0, stream, prm, a);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&c, sim.ctr, sizeof c, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (c.error) break;
            if (allow_stop) report_progress((uint32_t)rounds_done, c.generated, c.steps, c.walks);
            if (c.walks - walks_before >= n) { *complete = true; break; }
            if (allow_stop && stop_requested) break;
        }
        return MC_OK;
    }
    int simulate(const mc_sim_opts *o, mc_sim_result *out) override {
        memset(out, 0, sizeof *out);
        out->violated_invariant = -1;
        if (!o || o->depth < 1 || o->depth > MC_SIM_MAX_DEPTH || (o->record && (!o->record_slots || !o->record_len || !o->record_end))) {
            set_error("simulate: depth must be 1 .. MC_SIM_MAX_DEPTH, and a record request needs its three arrays");
            return MC_EBADCFG;
        }
        if (o->num > SIM_MAX_WALKS) { set_error("simulate: at most 2^40 walks"); return MC_EBADCFG; }
        if (cfg.shard_count > 1) { set_error("simulate: not available for a sharded engine"); return MC_EBADCFG; }
        // the BFS's resident search is no longer continued by mc_engine_step, nor checkpointed
        fr.have_run = fr.have_viol = false;
        ck.pending = ck.in_place = false;
        stop_requested = false;
        gr.release();
        sim.trace_n = 0;
        sim.trace_rows.clear();
        sim.trace_acts.clear();
        HIP_TRY(hipSetDevice(cfg.device));
        const uint64_t lanes = ((o->num && o->num < SIM_ROUND ? o->num : SIM_ROUND) + 63) & ~63ull;
        HIP_TRY(sim.buf[0].reserve(lanes * W));
        HIP_TRY(sim.buf[1].reserve(lanes * W));
        HIP_TRY(sim.wst.reserve(lanes));
        HIP_TRY(sim.ctr.reserve(1));
        int rc;
        const uint64_t K = o->record;
        DevBuf<int32_t> d_rslots, d_tslots;  // the recorded walks' slots (K walks) / the counterexample's (one walk)
        DevBuf<uint32_t> d_rlen, d_tlen;
        DevBuf<uint64_t> d_rows;
        if (K) {
            HIP_TRY(d_rslots.alloc(K * o->depth));
            HIP_TRY(d_rlen.alloc(2 * K));
            HIP_TRY(hipMemsetAsync(d_rslots, 0xff, K * o->depth * sizeof(int32_t), stream));
            HIP_TRY(hipMemsetAsync(d_rlen, 0, 2 * K * sizeof(uint32_t), stream));
        }
        SimCounters c;
        memset(&c, 0, sizeof c);
        c.viol = ~0ull;
        HIP_TRY(hipMemcpyAsync(sim.ctr, &c, sizeof c, hipMemcpyHostToDevice, stream));
        SimArgs a{};
        a.seed = o->seed;
        a.buf0 = sim.buf[0];
        a.buf1 = sim.buf[1];
        a.wst = sim.wst;
        a.depth = o->depth;
        a.iters = SIM_ITERS;
        a.deadlock = (cfg.flags & MC_F_DEADLOCK) ? 1u : 0u;
        a.ctr = sim.ctr;
        a.rec_first = 0;
        a.rec_count = K;
        a.rec_slots = d_rslots;
        a.rec_len = d_rlen;
        a.rec_end = d_rlen ? d_rlen + K : nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        progress_last = t0;
        bool stopped = false;
        uint64_t rounds = 0;
        for (uint64_t first = 0; !o->num || first < o->num; first += SIM_ROUND, ++rounds) {
            if (first >= SIM_MAX_WALKS) { stopped = true; break; }   // (num = 0: walk indices must stay below 2^40, the width of a key's walk field)
            const uint64_t n = o->num && o->num - first < SIM_ROUND ? o->num - first : SIM_ROUND;
            a.w0 = first;
            const uint64_t before = c.walks;
            bool complete = false;
            if ((rc = sim_round(a, n, c, before, true, rounds, &complete))) return rc;
            if (c.error & DEV_EOVERFLOW) { set_error("packed-state capacity exceeded (raft messages / elections / allLogs slots, or a PlusCal sequence longer than its cells, or a recursive PlusCal procedure deeper than $TLAMC_PCAL_STACK frames)"); return MC_EOVERFLOW; }
            // stopped inside a round: a violation among the walks that ended need not be the round's lowest-indexed one (a walk of a
            // lower index may not have ended yet), so none is reported — the run ends like a spent budget, as a stopped BFS does
            if (!complete) { stopped = true; c.viol = ~0ull; break; }
            if (c.viol != ~0ull) break;
            if (stop_requested) { stopped = true; break; }
        }
        out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        out->walks = c.walks;
        out->steps = c.steps;
        out->generated = c.generated;
        out->max_depth = c.max_depth;
        out->verdict = stopped ? MC_V_BUDGET : MC_V_OK;
        if (K) {
            HIP_TRY(hipMemcpy(o->record_slots, d_rslots, K * o->depth * sizeof(int32_t), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(o->record_len, d_rlen, K * sizeof(uint32_t), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(o->record_end, d_rlen + K, K * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        if (c.viol == ~0ull) return MC_OK;
        const unsigned long long key = c.viol;
        const unsigned kind = sim_key_kind(key), vslot = sim_key_slot(key);
        out->verdict = verdict_of_kind(kind);
        if (kind == SIM_VK_INVARIANT) out->violated_invariant = (int)sim_key_inv(key);
        out->violating_walk = sim_key_walk(key);
        // the counterexample: walk w once more, alone, in record mode (nothing was kept per walk in the run itself)
        HIP_TRY(d_tslots.alloc((size_t)o->depth));
        HIP_TRY(d_tlen.alloc(2));
        HIP_TRY(d_rows.alloc(((size_t)o->depth + 1) * W));
        HIP_TRY(hipMemsetAsync(d_tslots, 0xff, (size_t)o->depth * sizeof(int32_t), stream));
        SimCounters c2;
        memset(&c2, 0, sizeof c2);
        c2.viol = ~0ull;
        HIP_TRY(hipMemcpyAsync(sim.ctr, &c2, sizeof c2, hipMemcpyHostToDevice, stream));
        a.w0 = out->violating_walk;
        a.rec_first = out->violating_walk;
        a.rec_count = 1;
        a.rec_slots = d_tslots;
        a.rec_len = d_tlen;
        a.rec_end = d_tlen + 1;
        a.rec_rows = d_rows;
        bool complete = false;
        if ((rc = sim_round(a, 1, c2, 0, false, 0, &complete))) return rc;
        uint32_t len = 0;
        HIP_TRY(hipMemcpy(&len, d_tlen, sizeof len, hipMemcpyDeviceToHost));
        if (c2.viol != key || len < 1 || len > o->depth) { set_error("simulate: the violating walk did not repeat in record mode"); return MC_ESTATE; }
        const bool extra = kind == SIM_VK_INVARIANT && vslot < SIM_SLOT_PARENT;
        const size_t n = len + (extra ? 1u : 0u);
        std::vector<int32_t> slots(len > 1 ? len - 1 : 1);
        sim.trace_rows.resize(n * W);
        HIP_TRY(hipMemcpy(sim.trace_rows.data(), d_rows, n * W * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (len > 1) HIP_TRY(hipMemcpy(slots.data(), d_tslots, (len - 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
        sim.trace_acts.assign(1, -1);
        for (size_t k = 1; k < len; ++k) sim.trace_acts.push_back(S::action_of(prm, &sim.trace_rows[(k - 1) * W], slots[k - 1]));
        if (extra) sim.trace_acts.push_back(S::action_of(prm, &sim.trace_rows[(size_t)(len - 1) * W], (int)vslot));
        sim.trace_n = n;
        out->trace_len = (uint32_t)n;
        return MC_OK;
    }
    int sim_trace_out(uint8_t *states_out, int32_t *actions_out, size_t *n_inout) {
        const size_t n = sim.trace_n;
        if (n > *n_inout) { *n_inout = n; set_error("trace buffer too small"); return MC_EBADCFG; }
        if constexpr (HasExport<S>::value || RaftPacked<S>::value) {  // rows leave the engine in the spec's PUBLIC layout, as the BFS's traces do
            for (size_t k = 0; k < n; ++k) S::export_row(prm, &sim.trace_rows[k * W], (uint64_t *)states_out + k * export_words_of<S>(prm, W));
        } else
        memcpy(states_out, sim.trace_rows.data(), n * W * sizeof(uint64_t));
        memcpy(actions_out, sim.trace_acts.data(), n * sizeof(int32_t));
        *n_inout = n;
        return MC_OK;
    }
    // ------------------------------------------------------------------------------- behaviours (mc_engine_behaviours; engine_behaviours.h)
    // The batch runs in rounds of chunk / 64 behaviours (a behaviour takes 64 columns of each of three buffers: a round takes what three
    // chunks of states take), each round in ceil(longest behaviour / iters) launches, enqueued back to back: a launch is bounded by
    // `iters` observations per behaviour, and a decided behaviour's wavefront leaves at once.  Nothing of the search is touched.
    static constexpr uint32_t BEH_ITERS = 16;
    const mc_spec_desc *spec_desc() const override { return &desc; }
    int behaviours_refused() override {
        if (cfg.shard_count > 1) { set_error("behaviours: not available for a sharded engine (shard_count > 1)"); return MC_EBADCFG; }
        if (PackedRows<S>::value || HasExport<S>::value) {
            set_error("behaviours: not available for an MC_F_JIT engine: generated code packs its rows, and there is no import_row that turns an observation "
                      "in the interpreter's layout into one (create the engine without MC_F_JIT)");
            return MC_EBADCFG;
        }
        if (S::num_init(prm) > MC_BEH_MAX_INIT) { set_error("behaviours: the model has more than 65536 initial states"); return MC_EBADCFG; }
        return MC_OK;
    }
    int behaviours(const mc_beh_opts *o, mc_beh_verdict *out, mc_beh_result *res) override {
        memset(res, 0, sizeof *res);
        res->first_rejected = ~0ull;
        if (int rc = behaviours_refused()) return rc;
        if constexpr (PackedRows<S>::value || HasExport<S>::value) return MC_EBADCFG;
        else {
        if (o->count && (!o->first || !o->rows || !out)) { set_error("behaviours: first, rows and the verdict array are needed"); return MC_EBADCFG; }
        for (uint64_t b = 0; b < o->count; ++b)
            if (o->first[b + 1] <= o->first[b] || o->first[b + 1] - o->first[b] >= (1ull << 31)) {
                set_error("behaviours: behaviour " + std::to_string(b) + " is empty (T = 0), or longer than 2^31 - 1 observations");
                return MC_EBADCFG;
            }
        if (!o->count) return MC_OK;
        HIP_TRY(hipSetDevice(cfg.device));
        // (an early return leaves no copy into the caller's arrays or out of this frame's in flight)
        struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{stream};
        const uint32_t iters = o->iters ? o->iters : BEH_ITERS;
        const uint64_t R = chunk / 64 < o->count ? chunk / 64 : o->count;   // (chunk >= 256)
        // observations and the mask arrive in the PUBLIC layout; a lowering that stores narrower rows takes them through import_row
        const size_t PW = export_words_of<S>(prm, W);
        std::vector<uint64_t> hmask(PW, ~0ull), imported;
        if (o->mask) memcpy(hmask.data(), o->mask, PW * sizeof(uint64_t));
        const bool full = beh_mask_full(hmask.data(), (int)PW);
        if constexpr (RaftPacked<S>::value) {
            std::vector<uint64_t> pm(hmask);
            hmask.assign(W, 0);
            S::import_row(prm, pm.data(), hmask.data());
        }
        for (int k = 0; k < 2; ++k) HIP_TRY(beh.set[k].reserve(R * 64 * W));
        HIP_TRY(beh.stage.reserve(R * 64 * W));
        HIP_TRY(beh.first.reserve(R + 1));
        HIP_TRY(beh.carry.reserve(R));
        HIP_TRY(beh.out.reserve(R));
        HIP_TRY(beh.ctr.reserve(1));
        BehCounters c;
        memset(&c, 0, sizeof c);
        c.first_rejected = ~0ull;
        HIP_TRY(hipMemcpyAsync(beh.ctr, &c, sizeof c, hipMemcpyHostToDevice, stream));
        if (!full) {
            HIP_TRY(beh.mask.reserve(W));
            HIP_TRY(hipMemcpyAsync(beh.mask, hmask.data(), (size_t)W * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        }
        BehArgs a{};
        a.mask = full ? nullptr : (const uint64_t *)beh.mask;
        a.flags = o->flags;
        a.iters = iters;
        a.ctr = beh.ctr;
        // unlogged steps (MC_BEH_F_HIDDEN): the instantiation that closes a set under hidden steps, with LDS for it; without, the plain one
        const bool hidden = beh_hidden(o->flags) != 0;
        const size_t lds = beh_lds_words(W, hidden) * sizeof(uint64_t);
        std::vector<uint64_t> rel(R + 1);
        const auto t0 = std::chrono::steady_clock::now();
        for (uint64_t b0 = 0; b0 < o->count; b0 += R) {
            const uint64_t n = o->count - b0 < R ? o->count - b0 : R;
            const uint64_t r0 = o->first[b0], nrows = o->first[b0 + n] - r0;
            uint64_t longest = 0;
            for (uint64_t k = 0; k <= n; ++k) rel[k] = o->first[b0 + k] - r0;
            for (uint64_t k = 0; k < n; ++k) longest = std::max(longest, rel[k + 1] - rel[k]);
            HIP_TRY(beh.rows.reserve(nrows * W));
            if constexpr (RaftPacked<S>::value) {
                imported.resize(nrows * W);   // (read by the copy until the round's synchronisation below)
                for (uint64_t k = 0; k < nrows; ++k) S::import_row(prm, (const uint64_t *)o->rows + (r0 + k) * PW, &imported[k * W]);
                HIP_TRY(hipMemcpyAsync(beh.rows, imported.data(), nrows * W * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
            } else
            HIP_TRY(hipMemcpyAsync(beh.rows, o->rows + r0 * W * sizeof(uint64_t), nrows * W * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(beh.first, rel.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemsetAsync(beh.carry, 0, n * sizeof(uint64_t), stream));
            HIP_TRY(hipMemsetAsync(beh.out, 0, n * sizeof(mc_beh_verdict), stream));
            a.b0 = b0;
            a.n = n;
            a.first = beh.first;
            a.rows = beh.rows;
            a.set0 = beh.set[0];
            a.set1 = beh.set[1];
            a.stage = beh.stage;
            a.carry = beh.carry;
            a.out = beh.out;
            for (uint64_t l = 0; l < (longest + iters - 1) / iters; ++l) {
                if (hidden) hipLaunchKernelGGL((k_behaviours<S, 0, true>), dim3((unsigned)n), dim3(64), lds, stream, prm, a);
                else hipLaunchKernelGGL(k_behaviours<S>, dim3((unsigned)n), dim3(64), lds, stream, prm, a);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipMemcpyAsync(out + b0, beh.out, n * sizeof(mc_beh_verdict), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));   // (rel and the round's buffers are reused by the next round)
        }
        HIP_TRY(hipMemcpy(&c, beh.ctr, sizeof c, hipMemcpyDeviceToHost));
        res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        res->accepted = c.accepted;
        res->rejected = c.rejected;
        res->ambiguous = c.ambiguous;
        res->observations = c.observations;
        res->generated = c.generated;
        res->first_rejected = c.first_rejected;
        if (c.accepted + c.rejected + c.ambiguous != o->count) { set_error("behaviours: a behaviour was left undecided"); return MC_ESTATE; }
        return MC_OK;
        }
    }
    int kernel_stats(mc_kernel_stats *o) override {
        o->expand = kstat[0];
        o->insert = kstat[1];
        o->materialise = kstat[2];
        o->state_bytes = (uint64_t)W * 8;
        o->cand_cells = fr.cells;
        o->inwave_states = fr.inwave;
        return MC_OK;
    }
};

}  // namespace mc

// --------------------------------------------------------------------------------------- engine factories
// group 1: atomic_add + pcal_intro, 2: raft (2 servers), 3: raft (3), 4: raft (5), 5: serializableSnapshotIsolation,
// 6: compiled PlusCal, 7: Voting / Paxos
namespace mc {
static int spec_group(const mc_spec_desc *d) {
    if (!d) return 0;
    switch (d->spec_id) {
    case MC_SPEC_ATOMIC_ADD: case MC_SPEC_PCAL_INTRO: return 1;
    case MC_SPEC_RAFT: return d->nparams < 1 ? 0 : d->params[0] == 2 ? 2 : d->params[0] == 3 ? 3 : d->params[0] == 5 ? 4 : 0;
    case MC_SPEC_SSI: return 5;
    case MC_SPEC_PCAL: return 6;
    case MC_SPEC_PAXOS: return 7;
    default: return 0;
    }
}
template <class S>
static int make_engine(const typename S::Params &prm, const mc_spec_desc *spec, const mc_config *cfg, EngineBase **out) {
    auto *e = new Engine<S>();
    e->prm = prm;
    e->desc = *spec;
    e->cfg = *cfg;
    e->created_with = *cfg;
    const int r = e->alloc();
    if (r) { delete e; return r; }
    *out = e;
    return MC_OK;
}
}  // namespace mc
extern "C" {
int mc_make_engine_1(const mc_spec_desc *, const mc_config *, mc::EngineBase **);
int mc_make_engine_2(const mc_spec_desc *, const mc_config *, mc::EngineBase **);
int mc_make_engine_3(const mc_spec_desc *, const mc_config *, mc::EngineBase **);
int mc_make_engine_4(const mc_spec_desc *, const mc_config *, mc::EngineBase **);
int mc_make_engine_5(const mc_spec_desc *, const mc_config *, mc::EngineBase **);
int mc_make_engine_6(const mc_spec_desc *, const mc_config *, mc::EngineBase **);
int mc_make_engine_7(const mc_spec_desc *, const mc_config *, mc::EngineBase **);
int mc_make_engine_2p(const mc_spec_desc *, const mc_config *, mc::EngineBase **);   // raft with 2 / 3 servers over narrower stored rows (spec_raft_packed.h)
int mc_make_engine_3p(const mc_spec_desc *, const mc_config *, mc::EngineBase **);
void *mc_jit_factory_opts(const void *program, int pack);   // pcal_codegen.cpp: the factory of the engine library built from the program's generated code, or null
#if MC_TU == 1 || MC_TU == -1
int mc_make_engine_1(const mc_spec_desc *d, const mc_config *c, mc::EngineBase **out) {
    if (d->spec_id == MC_SPEC_ATOMIC_ADD) {
        mc::SpecAtomicAdd::Params p;
        if (mc::SpecAtomicAdd::make_params(d->params, d->nparams, p)) return MC_EBADCFG;
        return mc::make_engine<mc::SpecAtomicAdd>(p, d, c, out);
    }
    mc::SpecPcalIntro::Params p;
    if (mc::SpecPcalIntro::make_params(d->params, d->nparams, p)) return MC_EBADCFG;
    return mc::make_engine<mc::SpecPcalIntro>(p, d, c, out);
}
#endif
#define MC_RAFT_FACTORY(K, SPEC)                                                                   \
    int mc_make_engine_##K(const mc_spec_desc *d, const mc_config *c, mc::EngineBase **out) {      \
        mc::RaftParams p;                                                                          \
        if (mc::SPEC::make_params(d->params, d->nparams, p)) return MC_EBADCFG;                    \
        return mc::make_engine<mc::SPEC>(p, d, c, out);                                            \
    }
#if MC_TU == 2 || MC_TU == -1
MC_RAFT_FACTORY(2, SpecRaft2)
#endif
#if MC_TU == 3 || MC_TU == -1
MC_RAFT_FACTORY(3, SpecRaft3)
#endif
#if MC_TU == 4 || MC_TU == -1
MC_RAFT_FACTORY(4, SpecRaft5)
#endif
// ... over the packed rows: units of their own (the by-family kernels are instantiated once more)
#define MC_RAFT_PACKED_FACTORY(K, NSRV)                                                            \
    int mc_make_engine_##K##p(const mc_spec_desc *d, const mc_config *c, mc::EngineBase **out) {   \
        mc::RaftParams p;                                                                          \
        if (mc::SpecRaftPacked<NSRV>::make_params(d->params, d->nparams, p)) return MC_EBADCFG;    \
        if (!mc::SpecRaftPacked<NSRV>::packable(p) || c->shard_count > 1) return MC_EBADCFG;       \
        return mc::make_engine<mc::SpecRaftPacked<NSRV>>(p, d, c, out);                            \
    }
#if MC_TU == 12 || MC_TU == -1
MC_RAFT_PACKED_FACTORY(2, 2)
#endif
#if MC_TU == 13 || MC_TU == -1
MC_RAFT_PACKED_FACTORY(3, 3)
#endif
#if MC_TU == 5 || MC_TU == -1
int mc_make_engine_5(const mc_spec_desc *d, const mc_config *c, mc::EngineBase **out) {
    mc::SsiParams p;
    if (mc::SpecSsi::make_params(d->params, d->nparams, p)) return MC_EBADCFG;
    return mc::make_engine<mc::SpecSsi>(p, d, c, out);
}
#endif
#if MC_TU == 7 || MC_TU == -1
// Voting / Paxos (spec_paxos.h)
int mc_make_engine_7(const mc_spec_desc *d, const mc_config *c, mc::EngineBase **out) {
    mc::PaxosParams p;
    if (mc::SpecPaxos::make_params(d->params, d->nparams, p)) return MC_EBADCFG;
    return mc::make_engine<mc::SpecPaxos>(p, d, c, out);
}
#endif
#if MC_TU == 6 || MC_TU == -1
// compiled PlusCal (spec_vm.h): the program image is copied to the device, the kernels read it through prm.code
int mc_make_engine_6(const mc_spec_desc *d, const mc_config *c, mc::EngineBase **out) {
    mc::VmParams p;
    if (mc::vm_make_params(d->params, d->nparams, p)) return MC_EBADCFG;
    if (hipSetDevice(c->device) != hipSuccess) { mc::set_error("hipSetDevice failed"); return MC_EHIP; }
    mc::DevBuf<int32_t> d_code;
    const size_t image_words = (size_t)p.code_len + (size_t)mc::vm_ext_words(p);   // (with the table behind the image and the entries behind that: spec_vm_cfg.h VmExt)
    if (d_code.alloc(image_words) != hipSuccess ||
        hipMemcpy(d_code, p.code, image_words * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
        mc::set_error("cannot upload the PlusCal program image");
        return MC_EHIP;
    }
    // identity of the compiled program for checkpoints: the whole image (header, tables, code) and the scalars derived from it
    uint64_t ph = 0xcbf29ce484222325ull;
    auto mixin = [&](uint64_t v) { ph = (ph ^ v) * 0x100000001b3ull; ph ^= ph >> 29; };
    for (int i = 0; i < p.code_len; i++) mixin((uint32_t)p.code[i]);
    for (int v : {p.nv, p.words, p.ninst, p.maxch, p.pc_base, p.done, p.init_entry, p.ninv, p.ncon, p.label_tab, p.self_tab, p.code_len}) mixin((uint32_t)v);
    for (int i = 0; i < 8; i++) mixin((uint32_t)p.inv_entry[i]);
    mixin(p.num_init);
    if (p.code[p.code_len + mc::VMX_NACON] || p.code[p.code_len + mc::VMX_NVIEW])   // the cfg's ACTION_CONSTRAINTs / VIEW (their code is part of the image, their
        for (int i = 0; i < mc::vm_ext_words(p); i++) mixin((uint32_t)p.code[p.code_len + i]);   // table behind it, a PROPERTY's safety entries): a checkpoint under one is refused under another
    p.code = d_code;  // host-side helpers (format, action_of) use p.host only
    const int rc = p.nv <= 16 ? mc::make_engine<mc::SpecVmCfg16>(p, d, c, out)
                 : p.nv <= 32 ? mc::make_engine<mc::SpecVmCfg32>(p, d, c, out)
                 : p.nv <= 64 ? mc::make_engine<mc::SpecVmCfg64>(p, d, c, out) : mc::make_engine<mc::SpecVmCfg>(p, d, c, out);
    if (!rc) { (*out)->owned_device_blob = std::move(d_code); (*out)->program_hash = ph ? ph : 1; }
    return rc;
}
#endif
#if MC_TU == 9
// A compiled PlusCal program as GENERATED code (spec_gen.h; pcal_codegen.cpp writes the header and builds this translation unit into a
// library of its own when the engine is created: mc_jit_factory).  Same parameters, same packed states, same program identity as group 6.
}  // extern "C"
#include MC_GEN_HEADER
extern "C" {
int mc_make_engine_gen(const mc_spec_desc *d, const mc_config *c, mc::EngineBase **out) {
    mc::VmParams p;
    if (mc::SpecGen::make_params(d->params, d->nparams, p)) { mc::set_error("jit: the generated engine was built from another program"); return MC_EBADCFG; }
    uint64_t ph = 0xcbf29ce484222325ull;
    auto mixin = [&](uint64_t v) { ph = (ph ^ v) * 0x100000001b3ull; ph ^= ph >> 29; };
    for (int i = 0; i < p.code_len; i++) mixin((uint32_t)p.code[i]);
    for (int v : {p.nv, p.words, p.ninst, p.maxch, p.pc_base, p.done, p.init_entry, p.ninv, p.ncon, p.label_tab, p.self_tab, p.code_len}) mixin((uint32_t)v);
    for (int i = 0; i < 8; i++) mixin((uint32_t)p.inv_entry[i]);
    mixin(p.num_init);
    if (p.code[p.code_len + mc::VMX_NACON] || p.code[p.code_len + mc::VMX_NVIEW])   // the cfg's ACTION_CONSTRAINTs / VIEW (their code is part of the image, their
        for (int i = 0; i < mc::vm_ext_words(p); i++) mixin((uint32_t)p.code[p.code_len + i]);   // table behind it, a PROPERTY's safety entries): a checkpoint under one is refused under another
    p.code = nullptr;   // the device never reads the image: the program IS the kernels
    const int rc = mc::make_engine<mc::SpecGen>(p, d, c, out);
    if (mc::SpecGen::PACKED_ROWS) { mixin(0x7061636bu); mixin((uint32_t)mc::SpecGen::MAX_WORDS); }   // a checkpoint of packed rows is not the interpreter's
    if (!rc) (*out)->program_hash = ph ? ph : 1;
    return rc;
}
#endif
}  // extern "C"

#if MC_TU == 0 || MC_TU == -1
static thread_local std::string g_last_error;
// --------------------------------------------------------------------------------------- C ABI
using namespace mc;

struct mc_engine {
    EngineBase *impl;
};

// raft on ONE GPU stores its rows in fewer words where the model's constants let it (spec_raft_packed.h); $TLAMC_RAFT_PACK=0 = A/B: the rows of
// every other engine.  Engines of a sharded job (shard_count > 1) exchange rows between ranks and keep the public layout (include/tlamc.h).
static bool raft_rows_packed(const mc_spec_desc *spec, const mc_config *cfg) {
    const char *ep = getenv("TLAMC_RAFT_PACK");
    if ((ep && *ep == '0') || cfg->shard_count > 1 || spec->spec_id != MC_SPEC_RAFT || spec->nparams < 5) return false;
    RaftParams p;
    if (spec->params[0] == 2) return !SpecRaft2::make_params(spec->params, spec->nparams, p) && SpecRaftPacked<2>::packable(p);
    if (spec->params[0] == 3) return !SpecRaft3::make_params(spec->params, spec->nparams, p) && SpecRaftPacked<3>::packable(p);
    return false;
}
static int make_impl(const mc_spec_desc *spec, const mc_config *cfg, bool pack, EngineBase **impl);
// The engine the mc_shard_* calls act on.  A one-GPU raft engine that stores narrow rows and has not searched yet is made again with the
// rows the step calls exchange, behind its handle; one that has searched refuses the call (Engine::refuse_packed).
static EngineBase *shard_side(mc_engine *e) {
    if (e->impl->narrow_rows() != 1) return e->impl;
    const mc_spec_desc desc = *e->impl->spec_desc();
    const mc_config cfg = e->impl->created_with;
    mc_progress_fn fn = e->impl->progress_fn;
    void *user = e->impl->progress_user;
    const double interval = e->impl->progress_interval;
    EngineBase *impl = nullptr;
    if (make_impl(&desc, &cfg, false, &impl) != MC_OK) return e->impl;   // (no room for both for a moment: the call is refused, Engine::refuse_packed says how to go on)
    delete e->impl;
    impl->progress_fn = fn;
    impl->progress_user = user;
    impl->progress_interval = interval;
    e->impl = impl;
    return impl;
}

extern "C" {

int mc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mc_engine_create(const mc_spec_desc *spec, const mc_config *cfg, mc_engine **out) {
    if (!spec || !cfg || !out) return MC_EBADCFG;
    *out = nullptr;
    if (mc_device_count() <= 0) { set_error("no HIP device: libtlamc has no CPU fallback"); return MC_EHIP; }
    g_last_error.clear();
    mc_config with_trace;
    if (cfg->flags & MC_F_COVERAGE) {
        if (cfg->shard_count > 1) { set_error("MC_F_COVERAGE: not available for a sharded engine (shard_count > 1)"); return MC_EBADCFG; }
        with_trace = *cfg;
        with_trace.flags |= MC_F_TRACE;   // distinct[a] is read off the trace records
        cfg = &with_trace;
    }
    if (cfg->flags & MC_F_CONTINUE) {
        if (cfg->shard_count > 1) { set_error("MC_F_CONTINUE: not available for a sharded engine (shard_count > 1)"); return MC_EBADCFG; }
        with_trace = *cfg;
        with_trace.flags |= MC_F_TRACE;   // the stored pass re-evaluates the trace records; every entry has a behaviour
        cfg = &with_trace;
    }
    EngineBase *impl = nullptr;
    const int rc = make_impl(spec, cfg, raft_rows_packed(spec, cfg), &impl);
    if (rc == MC_OK) *out = new mc_engine{impl};
    else if (rc == MC_EBADCFG && g_last_error.empty()) set_error("unknown spec id or constants out of range");
    return rc;
}
}  // extern "C"
static int make_impl(const mc_spec_desc *spec, const mc_config *cfg, bool pack, EngineBase **out) {
    EngineBase *impl = nullptr;
    const int group = spec_group(spec);
    int rc = MC_EBADCFG;
    switch (group) {
    case 1: rc = mc_make_engine_1(spec, cfg, &impl); break;
    case 2: rc = pack ? mc_make_engine_2p(spec, cfg, &impl) : mc_make_engine_2(spec, cfg, &impl); break;
    case 3: rc = pack ? mc_make_engine_3p(spec, cfg, &impl) : mc_make_engine_3(spec, cfg, &impl); break;
    case 4: rc = mc_make_engine_4(spec, cfg, &impl); break;
    case 5: rc = mc_make_engine_5(spec, cfg, &impl); break;
    case 6: {
        // MC_F_JIT / $TLAMC_JIT: the program as generated, compiled code (pcal_codegen.cpp); the interpreter when that is not to be had
        const char *ej = getenv("TLAMC_JIT");
        rc = MC_EBADCFG;
        bool jit = false;
        if (((cfg->flags & MC_F_JIT) || (ej && *ej && *ej != '0')) && spec->nparams >= 1 && spec->params[0]) {
            typedef int (*factory_t)(const mc_spec_desc *, const mc_config *, EngineBase **);
            factory_t fn = (factory_t)mc_jit_factory_opts((const void *)(intptr_t)spec->params[0], cfg->shard_count > 1 ? 0 : 1);
            // (the library is there and ITS engine cannot be made — out of device memory, a bad configuration: the caller's error, the
            //  interpreter's engine would meet it too; the interpreter stands in only for generated code that is not to be had)
            if (fn) { rc = fn(spec, cfg, &impl); jit = true; }
            else fprintf(stderr, "tlamc: MC_F_JIT: %s; interpreting the program on the device instead\n", g_last_error.c_str());
        }
        if (!jit) rc = mc_make_engine_6(spec, cfg, &impl);
        break;
    }
    case 7: rc = mc_make_engine_7(spec, cfg, &impl); break;
    default: break;
    }
    if (rc == MC_OK) *out = impl;
    return rc;
}
extern "C" {
int mc_engine_run(mc_engine *e, mc_result *out) { return e && out ? e->impl->run(out) : MC_EBADCFG; }
int mc_engine_step(mc_engine *e, uint32_t levels, mc_result *out) { return e && out ? e->impl->step(levels, out) : MC_EBADCFG; }
int mc_engine_set_progress(mc_engine *e, mc_progress_fn fn, void *user, double min_interval_seconds) {
    if (!e) return MC_EBADCFG;
    e->impl->progress_fn = fn;
    e->impl->progress_user = user;
    e->impl->progress_interval = min_interval_seconds > 0 ? min_interval_seconds : 0.0;
    return MC_OK;
}
int mc_engine_request_stop(mc_engine *e) {
    if (!e) return MC_EBADCFG;
    e->impl->stop_requested = true;
    return MC_OK;
}
int mc_engine_trace(mc_engine *e, uint8_t *states_out, int32_t *actions_out, size_t *n_inout) {
    return e && n_inout ? e->impl->trace(states_out, actions_out, n_inout) : MC_EBADCFG;
}
int mc_engine_behaviours(mc_engine *e, const mc_beh_opts *opts, mc_beh_verdict *out, mc_beh_result *result) {
    return e && opts && result ? e->impl->behaviours(opts, out, result) : MC_EBADCFG;
}
// the witness with (obs_out) or without the unlogged steps: one host run of the rule with links, one walk back through them
static int behaviour_path(const char *who, mc_engine *e, const mc_beh_opts *opts, uint64_t b, uint8_t *states_out, int32_t *slots_out, uint32_t *obs_out,
                          size_t *n_inout) {
    const std::string w(who);
    if (!e || !opts || !n_inout || !opts->first || !opts->rows || b >= opts->count || opts->first[b + 1] <= opts->first[b]) {
        mc_set_error_internal((w + ": no such behaviour").c_str());
        return MC_EBADCFG;
    }
    if (int rc = e->impl->behaviours_refused()) return rc;   // (what the batch call refuses)
    return dispatch_spec(e->impl->spec_desc(), [&](auto s, const auto &prm) {
        using S = decltype(s);
        const size_t W = (size_t)S::words(prm);
        const uint64_t T = opts->first[b + 1] - opts->first[b];
        std::vector<uint64_t> rows(T * W), mask(W);
        memcpy(rows.data(), opts->rows + opts->first[b] * W * sizeof(uint64_t), T * W * sizeof(uint64_t));
        if (opts->mask) memcpy(mask.data(), opts->mask, W * sizeof(uint64_t));
        mc_beh_verdict v;
        BehSets sets;
        beh_check<S>(prm, rows.data(), T, opts->mask ? mask.data() : nullptr, opts->flags, &v, &sets);
        const BehPath path = beh_path(sets, (int)W);
        const size_t n = path.slots.size();
        if (n > *n_inout) { *n_inout = n; mc_set_error_internal((w + ": buffers too small").c_str()); return MC_EBADCFG; }
        *n_inout = n;
        if (!n) return MC_OK;
        if (!states_out || !slots_out || !obs_out) { mc_set_error_internal((w + ": states_out, slots_out and obs_out are needed").c_str()); return MC_EBADCFG; }
        memcpy(states_out, path.states.data(), n * W * sizeof(uint64_t));
        memcpy(slots_out, path.slots.data(), n * sizeof(int32_t));
        memcpy(obs_out, path.obs.data(), n * sizeof(uint32_t));
        return MC_OK;
    });
}
int mc_engine_behaviour_path(mc_engine *e, const mc_beh_opts *opts, uint64_t b, uint8_t *states_out, int32_t *slots_out, uint32_t *obs_out, size_t *n_inout) {
    return behaviour_path("behaviour_path", e, opts, b, states_out, slots_out, obs_out, n_inout);
}
int mc_engine_behaviour_witness(mc_engine *e, const mc_beh_opts *opts, uint64_t b, uint8_t *states_out, int32_t *slots_out, size_t *n_inout) {
    if (!e || !opts || !n_inout || !opts->first || !opts->rows || b >= opts->count || opts->first[b + 1] <= opts->first[b]) {
        mc_set_error_internal("behaviour_witness: no such behaviour");
        return MC_EBADCFG;
    }
    if (beh_hidden(opts->flags)) {
        mc_set_error_internal("behaviour_witness: with unlogged steps (MC_BEH_F_HIDDEN) a path is longer than the log: call mc_engine_behaviour_path");
        return MC_EBADCFG;
    }
    if (int rc = e->impl->behaviours_refused()) return rc;   // (what the batch call refuses)
    return dispatch_spec(e->impl->spec_desc(), [&](auto s, const auto &prm) {
        using S = decltype(s);
        const size_t W = (size_t)S::words(prm);
        const uint64_t T = opts->first[b + 1] - opts->first[b];
        std::vector<uint64_t> rows(T * W), mask(W);
        memcpy(rows.data(), opts->rows + opts->first[b] * W * sizeof(uint64_t), T * W * sizeof(uint64_t));
        if (opts->mask) memcpy(mask.data(), opts->mask, W * sizeof(uint64_t));
        mc_beh_verdict v;
        BehSets sets;
        beh_check<S>(prm, rows.data(), T, opts->mask ? mask.data() : nullptr, opts->flags, &v, &sets);
        const size_t n = sets.sets.size();
        if (n > *n_inout) { *n_inout = n; mc_set_error_internal("behaviour_witness: buffers too small"); return MC_EBADCFG; }
        *n_inout = n;
        if (!n) return MC_OK;
        if (!states_out || !slots_out) { mc_set_error_internal("behaviour_witness: states_out and slots_out are needed"); return MC_EBADCFG; }
        std::vector<uint64_t> path(n * W);
        beh_witness(sets, (int)W, path.data(), slots_out);
        memcpy(states_out, path.data(), n * W * sizeof(uint64_t));
        return MC_OK;
    });
}
int mc_engine_simulate(mc_engine *e, const mc_sim_opts *opts, mc_sim_result *out) {
    return e && opts && out ? e->impl->simulate(opts, out) : MC_EBADCFG;
}
int mc_engine_coverage(mc_engine *e, mc_action_coverage *out, size_t *n_inout) { return e && n_inout ? e->impl->coverage(out, n_inout) : MC_EBADCFG; }
int mc_engine_violations(mc_engine *e, mc_violations_info *info, mc_violation *out, size_t *n_inout) {
    return e && n_inout ? e->impl->violations(info, out, n_inout) : MC_EBADCFG;
}
int mc_engine_violation_trace(mc_engine *e, size_t k, uint8_t *states_out, int32_t *actions_out, size_t *n_inout) {
    return e && n_inout ? e->impl->violation_trace(k, states_out, actions_out, n_inout) : MC_EBADCFG;
}
int mc_engine_graph(mc_engine *e, mc_graph_info *out) { return e && out ? e->impl->graph(out) : MC_EBADCFG; }
int mc_engine_graph_read(mc_engine *e, uint64_t first, uint64_t count, uint64_t *offsets_out, uint32_t *dst_out, int32_t *action_out, size_t *nedges_inout) {
    return e && nedges_inout ? e->impl->graph_read(first, count, offsets_out, dst_out, action_out, nedges_inout) : MC_EBADCFG;
}
int mc_engine_scc(mc_engine *e, mc_scc_info *out) { return e && out ? e->impl->scc(out) : MC_EBADCFG; }
int mc_engine_scc_read(mc_engine *e, uint64_t first, uint64_t count, uint32_t *scc_out) {
    return e && (scc_out || !count) ? e->impl->scc_read(first, count, scc_out) : MC_EBADCFG;
}
int mc_engine_predicates(mc_engine *e, uint64_t first, uint64_t count, uint32_t *bits_out) {
    return e && (bits_out || !count) ? e->impl->predicates(first, count, bits_out) : MC_EBADCFG;
}
// The six liveness checks: each is its LiveQuery (live_query.h) and the outputs it has.  prop null: Termination; `all` is the engine's to say.
static LiveQuery live_query_procs(const char *call, uint64_t weak, uint64_t strong, const mc_live_property *prop, bool refine) {
    return LiveQuery{call, 0, weak, strong, nullptr, prop ? prop->kind : -1, prop ? prop->p : -1, prop ? prop->q : -1, refine};
}
int mc_engine_liveness(mc_engine *e, uint64_t weak_fair_mask, mc_live_info *out) {
    return e && out ? e->impl->liveness_run(live_query_procs("mc_engine_liveness", weak_fair_mask, 0, nullptr, false), nullptr, out, nullptr, nullptr) : MC_EBADCFG;
}
int mc_engine_liveness_check(mc_engine *e, uint64_t weak_fair_mask, const mc_live_property *prop, mc_live_check_info *out) {
    return e && prop && out ? e->impl->liveness_run(live_query_procs("mc_engine_liveness_check", weak_fair_mask, 0, prop, false), prop, nullptr, out, nullptr) : MC_EBADCFG;
}
int mc_engine_liveness_strong(mc_engine *e, uint64_t weak_mask, uint64_t strong_mask, mc_live_info *out, mc_live_strong_info *strong_out) {
    return e && out && strong_out ? e->impl->liveness_run(live_query_procs("mc_engine_liveness_strong", weak_mask, strong_mask, nullptr, true), nullptr, out, nullptr, strong_out)
                                  : MC_EBADCFG;
}
int mc_engine_liveness_check_strong(mc_engine *e, uint64_t weak_mask, uint64_t strong_mask, const mc_live_property *prop, mc_live_check_info *out,
                                    mc_live_strong_info *strong_out) {
    return e && prop && out && strong_out
               ? e->impl->liveness_run(live_query_procs("mc_engine_liveness_check_strong", weak_mask, strong_mask, prop, true), prop, nullptr, out, strong_out)
               : MC_EBADCFG;
}
int mc_engine_liveness_units(mc_engine *e, const mc_fair_units *fu, mc_live_info *out, mc_live_strong_info *strong_out) {
    return e && fu && out && strong_out ? e->impl->liveness_run(live_query_units("mc_engine_liveness_units", fu, -1, -1, -1), nullptr, out, nullptr, strong_out) : MC_EBADCFG;
}
int mc_engine_liveness_check_units(mc_engine *e, const mc_fair_units *fu, const mc_live_property *prop, mc_live_check_info *out,
                                   mc_live_strong_info *strong_out) {
    return e && fu && prop && out && strong_out
               ? e->impl->liveness_run(live_query_units("mc_engine_liveness_check_units", fu, prop->kind, prop->p, prop->q), prop, nullptr, out, strong_out)
               : MC_EBADCFG;
}
int mc_engine_liveness_edge_units(mc_engine *e, uint64_t first_edge, uint64_t count, int8_t *unit_out) {
    return e && (unit_out || !count) ? e->impl->liveness_edge_units(first_edge, count, unit_out) : MC_EBADCFG;
}
int mc_engine_liveness_components(mc_engine *e, uint64_t first, uint64_t count, uint32_t *scc_out) {
    return e && (scc_out || !count) ? e->impl->liveness_components(first, count, scc_out) : MC_EBADCFG;
}
int mc_engine_liveness_trace(mc_engine *e, uint32_t *prefix_out, size_t *nprefix_inout, uint32_t *cycle_out, size_t *ncycle_inout) {
    return e && nprefix_inout && ncycle_inout ? e->impl->liveness_trace(prefix_out, nprefix_inout, cycle_out, ncycle_inout) : MC_EBADCFG;
}
int mc_engine_kernel_stats(mc_engine *e, mc_kernel_stats *out) { return e && out ? e->impl->kernel_stats(out) : MC_EBADCFG; }
int mc_engine_read_states(mc_engine *e, uint64_t first, uint64_t count, uint8_t *out) {
    return e && (out || !count) ? e->impl->read_states(first, count, out) : MC_EBADCFG;
}
int mc_engine_checkpoint(mc_engine *e, const char *path) { return e && path ? e->impl->checkpoint(path) : MC_EBADCFG; }
int mc_engine_restore(mc_engine *e, const char *path) { return e && path ? e->impl->restore(path) : MC_EBADCFG; }
void mc_engine_destroy(mc_engine *e) {
    if (!e) return;
    delete e->impl;
    delete e;
}

size_t mc_state_bytes(const mc_spec_desc *spec) {
    size_t n = 0;
    dispatch_spec(spec, [&](auto s, const auto &prm) { n = sizeof(uint64_t) * decltype(s)::words(prm); return 0; });
    return n;
}
uint32_t mc_fp_owner(uint64_t fp, uint32_t shard_count) { return fp_owner(fp, shard_count); }
int mc_state_format(const mc_spec_desc *spec, const uint8_t *state, char *buf, size_t cap) {
    if (!state || !buf || !cap) return MC_EBADCFG;
    int n = MC_EBADCFG;
    int rc = dispatch_spec(spec, [&](auto s, const auto &prm) {
        using S = decltype(s);
        uint64_t w[S::MAX_WORDS];
        memcpy(w, state, sizeof(uint64_t) * S::words(prm));
        n = S::format(prm, w, buf, cap);
        if ((size_t)n < cap) buf[n] = 0; else buf[cap - 1] = 0;
        return 0;
    });
    return rc ? rc : n;
}
// host-side evaluation of one (state, slot) pair: the action it is (mc_action_name's argument) and its successor
int mc_state_action(const mc_spec_desc *spec, const uint8_t *state, int32_t slot) {
    if (!state) return MC_EBADCFG;
    int a = -1;
    int rc = dispatch_spec(spec, [&](auto s, const auto &prm) {
        using S = decltype(s);
        uint64_t w[S::MAX_WORDS];
        memcpy(w, state, sizeof(uint64_t) * S::words(prm));
        a = S::action_of(prm, w, (int)slot);
        return 0;
    });
    return rc ? rc : a;
}
int mc_state_apply(const mc_spec_desc *spec, const uint8_t *state, int32_t slot, uint8_t *successor_out) {
    if (!state || !successor_out) return MC_EBADCFG;
    return dispatch_spec(spec, [&](auto s, const auto &prm) {
        using S = decltype(s);
        uint64_t w[S::MAX_WORDS], o[S::MAX_WORDS];
        memcpy(w, state, sizeof(uint64_t) * S::words(prm));
        S::apply(prm, CWordRef{w, 1}, (int)slot, WordRef{o, 1});
        memcpy(successor_out, o, sizeof(uint64_t) * S::words(prm));
        return 0;
    });
}
const char *mc_action_name(const mc_spec_desc *spec, int32_t action) {
    const char *nm = "?";
    dispatch_spec(spec, [&](auto s, const auto &prm) {
        if constexpr (std::is_same_v<std::decay_t<decltype(prm)>, VmParams>) nm = vm_action_name(prm.host, action);  // label names live in the program
        else nm = decltype(s)::action_name(action);
        return 0;
    });
    return nm;
}
const char *mc_strerror(int code) {
    switch (code) {
    case MC_OK: return "ok";
    case MC_EBADCFG: return "bad spec or configuration";
    case MC_EHIP: return "HIP error / no device";
    case MC_EOVERFLOW: return "packed-state slot array overflow";
    case MC_ETABLEFULL: return "seen-set full";
    case MC_EARENA: return "state arena full";
    case MC_ERCCL: return "exchange failure";
    case MC_ESTATE: return "call sequence error";
    case MC_EPARSE: return "parse error";
    case MC_ENOSPEC: return "module is not a lowered spec";
    case MC_EROUTE: return "exchange bucket full";
    default: return "unknown error";
    }
}
const char *mc_last_error(void) { return g_last_error.c_str(); }
void mc_set_error_internal(const char *msg) { g_last_error = msg ? msg : ""; }


int mc_engine_debug_reexpand(mc_engine *e, unsigned extra_flags, double *ms) { return e && ms ? e->impl->debug_reexpand(extra_flags, ms) : MC_EBADCFG; }
// profiling builds only (-DMC_PHASE_PROF): cycles per phase of k_expand_family summed over all wavefronts since the last reset
int mc_engine_debug_phases(mc_engine *e, uint64_t *out48, int reset) { return e && out48 ? e->impl->debug_phases(out48, reset) : MC_EBADCFG; }
int mc_engine_debug_flags(mc_engine *e, uint32_t set, uint32_t clear) { return e ? e->impl->debug_flags(set, clear) : MC_EBADCFG; }
int mc_engine_seen_layout(mc_engine *e, uint64_t *buckets, uint32_t *slots) { return e && buckets && slots ? e->impl->seen_layout(buckets, slots) : MC_EBADCFG; }
// ---- sharded (multi-GPU) step API
int mc_shard_begin(mc_engine *e) { return e ? shard_side(e)->shard_begin() : MC_EBADCFG; }
int mc_shard_begin_replicated(mc_engine *e, uint64_t min_frontier, uint64_t max_distinct, uint64_t max_levels, uint64_t *levels_out,
                              uint32_t *nlevels) {
    return e && levels_out && nlevels ? shard_side(e)->shard_begin_replicated(min_frontier, max_distinct, max_levels, levels_out, nlevels) : MC_EBADCFG;
}
int mc_shard_level_size(mc_engine *e, uint64_t *n) { return e && n ? shard_side(e)->shard_level_size(n) : MC_EBADCFG; }
int mc_shard_info(mc_engine *e, void **main_stream_out, uint64_t *chunk_states_out, int32_t *traced_out) {
    return e ? shard_side(e)->shard_info(main_stream_out, chunk_states_out, traced_out) : MC_EBADCFG;
}
size_t mc_engine_state_bytes_internal(mc_engine *e) { return e ? shard_side(e)->state_bytes() : 0; }
int mc_shard_expand(mc_engine *e, uint64_t first, uint64_t count, uint64_t *send_fp, uint64_t send_cap, uint64_t *send_counts) {
    if (!e || !send_counts) return MC_EBADCFG;
    const int rc = shard_side(e)->shard_expand_launch(0, first, count, send_cap);
    return rc ? rc : shard_side(e)->shard_expand_finish(0, send_fp, send_cap, send_counts);
}
int mc_shard_set_stream(mc_engine *e, void *hip_stream, int enable) { return e ? shard_side(e)->shard_set_stream(hip_stream, enable) : MC_EBADCFG; }
int mc_shard_expand_launch(mc_engine *e, uint32_t slot, uint64_t first, uint64_t count, uint64_t send_cap) {
    return e ? shard_side(e)->shard_expand_launch(slot, first, count, send_cap) : MC_EBADCFG;
}
int mc_shard_expand_finish(mc_engine *e, uint32_t slot, uint64_t *send_fp, uint64_t send_cap, uint64_t *send_counts) {
    return e && send_counts ? shard_side(e)->shard_expand_finish(slot, send_fp, send_cap, send_counts) : MC_EBADCFG;
}
int mc_shard_probe(mc_engine *e, const uint64_t *recv_fp, uint64_t n, uint8_t *answers) {
    return e ? shard_side(e)->shard_probe(recv_fp, n, answers) : MC_EBADCFG;
}
int mc_shard_materialise(mc_engine *e, const uint8_t *answers_back, uint8_t *send_states, uint64_t send_cap, uint64_t *send_counts) {
    return e && send_counts ? shard_side(e)->shard_materialise(0, answers_back, send_states, send_cap, send_counts) : MC_EBADCFG;
}
int mc_shard_materialise_slot(mc_engine *e, uint32_t slot, const uint8_t *answers_back, uint8_t *send_states, uint64_t send_cap,
                              uint64_t *send_counts) {
    return e && send_counts ? shard_side(e)->shard_materialise(slot, answers_back, send_states, send_cap, send_counts) : MC_EBADCFG;
}
int mc_shard_ingest(mc_engine *e, const uint8_t *recv_states, uint64_t n) { return e ? shard_side(e)->shard_ingest(recv_states, n) : MC_EBADCFG; }
int mc_shard_expand_pack(mc_engine *e, uint32_t slot, uint64_t *send_fp, uint64_t cap) { return e && send_fp ? shard_side(e)->shard_expand_pack(slot, send_fp, cap) : MC_EBADCFG; }
int mc_shard_probe_pack(mc_engine *e, const uint64_t *recv_fp, uint64_t cap, uint8_t *answers) {
    return e && recv_fp && answers ? shard_side(e)->shard_probe_pack(recv_fp, cap, answers) : MC_EBADCFG;
}
int mc_shard_keep_pack(mc_engine *e, uint32_t slot, const uint8_t *answers_back, uint64_t cap) {
    return e && answers_back ? shard_side(e)->shard_keep_pack(slot, answers_back, cap) : MC_EBADCFG;
}
int mc_shard_wait_keep(mc_engine *e, uint32_t slot) { return e ? shard_side(e)->shard_wait_keep(slot) : MC_EBADCFG; }
int mc_shard_keep(mc_engine *e, const uint8_t *answers_back, uint64_t *n_new) { return e && n_new ? shard_side(e)->shard_keep(0, answers_back, n_new) : MC_EBADCFG; }
int mc_shard_keep_slot(mc_engine *e, uint32_t slot, const uint8_t *answers_back, uint64_t *n_new) {
    return e ? shard_side(e)->shard_keep(slot, answers_back, n_new) : MC_EBADCFG;
}
int mc_shard_end_level(mc_engine *e, uint64_t *new_local) { return e && new_local ? shard_side(e)->shard_end_level(new_local) : MC_EBADCFG; }
int mc_shard_counters(mc_engine *e, uint64_t *generated, uint64_t *distinct_local, int32_t *verdict) {
    return e && generated && distinct_local && verdict ? shard_side(e)->shard_counters(generated, distinct_local, verdict) : MC_EBADCFG;
}
int mc_shard_check_frontier(mc_engine *e) { return e ? shard_side(e)->shard_check_frontier() : MC_EBADCFG; }
int mc_shard_materialise_parents(mc_engine *e, uint32_t slot, uint64_t *send_parents) { return e ? shard_side(e)->shard_materialise_parents(slot, send_parents) : MC_EBADCFG; }
int mc_shard_ingest_parents(mc_engine *e, const uint64_t *recv_parents, uint64_t n, uint32_t src_rank) {
    return e ? shard_side(e)->shard_ingest_parents(recv_parents, n, src_rank) : MC_EBADCFG;
}
int mc_shard_violation(mc_engine *e, int32_t *found, uint64_t *idx, uint32_t *slot, int32_t *verdict, int32_t *invariant) {
    return e && found && idx && slot && verdict && invariant ? shard_side(e)->shard_violation(found, idx, slot, verdict, invariant) : MC_EBADCFG;
}
int mc_shard_note_levels(mc_engine *e, const uint64_t *levels, uint32_t n, int32_t verdict) { return e && (levels || !n) ? shard_side(e)->shard_note_levels(levels, n, verdict) : MC_EBADCFG; }
int mc_shard_resume(mc_engine *e, uint64_t *levels_out, uint32_t *nlevels) { return e && levels_out && nlevels ? shard_side(e)->shard_resume(levels_out, nlevels) : MC_EBADCFG; }
int mc_shard_checkpoint(mc_engine *e, const char *path) { return e && path ? shard_side(e)->shard_checkpoint(path) : MC_EBADCFG; }
int mc_shard_restore(mc_engine *e, const char *path) { return e && path ? shard_side(e)->shard_restore(path) : MC_EBADCFG; }
int mc_shard_fetch(mc_engine *e, uint64_t idx, uint8_t *state_out, uint32_t *parent_rank, uint64_t *parent_idx, uint32_t *parent_slot) {
    return e && state_out && parent_rank && parent_idx && parent_slot ? shard_side(e)->shard_fetch(idx, state_out, parent_rank, parent_idx, parent_slot) : MC_EBADCFG;
}

}  // extern "C"
#endif  // MC_TU == 0 || MC_TU == -1
