// state_graph.h — the state graph of a finished search (mc_engine_graph) and what is computed from its CSR arrays alone: the reads, the
// strongly connected components (mc_engine_scc), the liveness checks (mc_engine_liveness and its five siblings: ONE entry, live_check,
// over a LiveQuery of live_query.h) and their counterexample.  None of it depends on the lowering, so the host half (state_graph.hip)
// and the kernels (engine_live.h) are compiled once for the library; the engine of every lowering — the one of generated code, built
// at load time, included — fills the arrays with its own kernels (engine_graph.h: k_graph_index / k_graph_degree / k_graph_fill /
// k_live_proc / k_live_unit / k_live_pred) and calls in here.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tlamc.h"
#include "hip_owned.h"
#include "live_query.h"   // LiveQuery: which check; liveness.h: LiveCheck and the LIVE_* bounds

namespace mc {

struct LiveCounters;   // engine_live.h

// `count` elements for a graph array; the message names the call and the array
template <class T>
int graph_alloc(DevBuf<T> &b, size_t count, const char *what, const char *call = "mc_engine_graph") {
    if (b.alloc(count ? count : 1) == hipSuccess) return MC_OK;
    (void)hipGetLastError();   // (the failed allocation is reported here, not by the next HIP call)
    set_error(std::string(call) + ": cannot allocate " + std::to_string((unsigned long long)(count * sizeof(T))) + " bytes of device memory for " + what);
    return MC_EARENA;
}

// The library's device scans.  out[i] = in[0] + ... + in[i - 1] in 64 bits, n items (degrees -> row offsets: the graph build and the
// transpose); `tmp` is (re)allocated to the scan's needs, `call` names the caller in the message of a failed allocation.
int scan_exclusive_u32_to_u64(const uint32_t *in, uint64_t *out, uint64_t n, DevBuf<char> &tmp, hipStream_t stream, const char *call);
// incl[i] = the number of non-zero answers among answers[0..i] (the sharded engine's keep step); `tmp` grows to the scan's needs
int scan_answers_inclusive(const uint8_t *answers, uint32_t *incl, uint64_t n, DevBuf<char> &tmp, hipStream_t stream);

// Built on demand from the arena and the seen-set a search left, gone with the next search (run / step / simulate / restore) or with
// the engine.
struct StateGraph {
    int device = 0;             // where the arrays live (the engine's device: set by the build)
    bool built = false;
    DevBuf<uint64_t> offsets;   // [states + 1]: row i of dst / act is [offsets[i], offsets[i + 1]); doubles as the out-degree table
    DevBuf<uint32_t> dst;       // [edges] arena index of the successor
    DevBuf<int16_t> act;        // [edges] action id (CovAction<S>::of: mc_action_name's)
    mc_graph_info info{};
    // what mc_engine_scc / mc_engine_liveness add: lives and dies with the graph
    struct Live {
        bool scc_built = false;
        DevBuf<uint64_t> toff;      // [states + 1] rows of the transpose (self loops left out)
        DevBuf<uint32_t> tsrc;      // [edges that are no self loops] the sources
        DevBuf<uint32_t> scc;       // [states] the least arena index of the state's component
        DevBuf<uint32_t> size;      // [states] at a component's id: its number of states
        DevBuf<int8_t> proc;        // [edges] beside act: the process instance that takes the edge, LIVE_TERM for the terminating disjunct
        DevBuf<unsigned long long> taken, disabled;   // [states] at a component's id: the unions over its states
        DevBuf<unsigned> done;      // [states] at a component's id: it holds a Done state
        mc_scc_info sinfo{};
        // what mc_engine_predicates / mc_engine_liveness_check add
        bool pred_built = false, proc_built = false;
        int npred = 0;              // the predicates pred[] has bits of (set with pred_built)
        DevBuf<uint32_t> pred;      // [states] bit k = predicate k of the program's temporal properties holds in the state
        DevBuf<uint32_t> dist;      // [states] the reach pass of the last check
        struct Masked { int q; DevBuf<uint32_t> scc, size; };   // the components of the subgraph induced by ~predicate q: one build per mask
        std::vector<std::unique_ptr<Masked>> masks;
        // what mc_engine_liveness_strong / mc_engine_liveness_check_strong add
        DevBuf<unsigned long long> enabled;    // [states] at a component's id: the processes enabled in some state of it
        DevBuf<uint8_t> open;                  // [states] LIVE_ST_*: closed, open or in a final component
        DevBuf<uint32_t> fscc, fsize;          // [states] the refined ids (a closed state: its own index) and, at an id, the size
        DevBuf<uint32_t> wscc, wsize;          // [states] the components of the open subgraph, rounds >= 2
        // what mc_engine_liveness_units / mc_engine_liveness_check_units add
        bool unit_built = false;
        DevBuf<int8_t> unit;                   // [edges] beside proc: the edge's unit (k_live_unit<S>), LIVE_TERM for the terminating disjunct
        DevBuf<uint64_t> of_unit;              // [LIVE_UNIT_TAB] the conjuncts of every unit, as the kernels stage it
        std::vector<uint64_t> of_unit_host;    // the same, for the counterexample builder
        // The last check, for mc_engine_liveness_components and the counterexample.  Value-reset where a check starts and in release(),
        // nowhere else; a check fills it as it goes and sets `checked` last.
        struct Last {
            bool checked = false;
            int kind = -1, p = -1, q = -1;      // -1 = Termination, else the kind of a property check and its (normalised) predicates
            bool refined = false;               // it ran the refinement: its components are fscc's
            bool units = false;                 // it read unit[] in proc[]'s place: fair / strong are masks of conjuncts
            uint64_t fair = 0, strong = 0;      // the weakly / strongly fair processes (conjuncts)
            const Masked *mask = nullptr;       // the components it judged (null: the full graph's)
            std::vector<uint32_t> descent;      // from the witness along falling dist to the first state of the component
            mc_live_info linfo{};               // the verdict: what the trace starts from
        } last;
        void release() {
            scc_built = pred_built = proc_built = unit_built = false;
            npred = 0;
            toff.reset(); tsrc.reset(); scc.reset(); size.reset(); proc.reset(); taken.reset(); disabled.reset(); done.reset();
            pred.reset(); dist.reset(); masks.clear();
            enabled.reset(); open.reset(); fscc.reset(); fsize.reset(); wscc.reset(); wsize.reset();
            unit.reset(); of_unit.reset(); of_unit_host.clear();
            last = Last{};
        }
    } lv;
    void release() { built = false; offsets.reset(); dst.reset(); act.reset(); lv.release(); }

    // mc_engine_graph_read
    int read(uint64_t first, uint64_t count, uint64_t *offsets_out, uint32_t *dst_out, int32_t *action_out, size_t *nedges_inout);
    // mc_engine_scc on a built graph, mc_engine_scc_read
    int scc(hipStream_t stream, mc_scc_info *out);
    int scc_read(uint64_t first, uint64_t count, uint32_t *scc_out);
    // mc_engine_predicates once the engine's k_live_pred<S> has filled lv.pred
    int pred_read(uint64_t first, uint64_t count, uint32_t *bits_out);
    // Every liveness check (live_query.h says which), once the components are found and what the query reads is there or enqueued on
    // `stream`: lv.proc (with q.fu: lv.unit) and, for a property, lv.pred with lv.npred.  Refuses what live_query_error refuses.
    // started: when the call began (the infos' seconds).  Of the outputs only those that apply may be non-null: lout for Termination,
    // cout for a property, sout with q.refine.
    int live_check(const LiveQuery &q, hipStream_t stream, std::chrono::steady_clock::time_point started, mc_live_info *lout, mc_live_check_info *cout,
                   mc_live_strong_info *sout);
    int live_scc_read(uint64_t first, uint64_t count, uint32_t *scc_out);   // mc_engine_liveness_components
    int live_unit_read(uint64_t first, uint64_t count, int8_t *unit_out);   // mc_engine_liveness_edge_units
    // mc_engine_liveness_trace; level_start: the search's level table (arena index of each BFS level's first state)
    int live_trace(const std::vector<uint64_t> &level_start, uint32_t *prefix_out, size_t *nprefix_inout, uint32_t *cycle_out, size_t *ncycle_inout);

private:
    int scc_build(uint64_t n, hipStream_t stream);
    // trim + colouring over the transpose that is there; mask: the predicate whose states are left out (a component of their own each), -1 = none
    // open: (rounds >= 2 of a strong check) only the states with LIVE_ST_OPEN there take part, in place of a predicate mask
    int scc_components(uint64_t n, hipStream_t stream, int mask_q, DevBuf<uint32_t> &scc_buf, DevBuf<uint32_t> &size_buf, mc_scc_info &info,
                       const uint8_t *open = nullptr);
    int live_mask_components(int kind, int q, hipStream_t stream, const Live::Masked **mask_out, uint32_t *builds);
    // the pieces of live_check (state_graph.hip)
    int live_single(const LiveQuery &q, hipStream_t stream, std::chrono::steady_clock::time_point started, mc_live_info *lout, mc_live_check_info *cout);
    int live_refined(const LiveQuery &q, hipStream_t stream, std::chrono::steady_clock::time_point started, mc_live_info *lout, mc_live_check_info *cout,
                     mc_live_strong_info *sout);
    int live_arrays(const LiveQuery &q);
    int live_clear(const LiveQuery &q, hipStream_t stream);
    void live_reduce(const LiveQuery &q, hipStream_t stream, const uint32_t *scc, const uint32_t *size, const LiveCheck &ck);
    int live_termination(uint64_t violating, uint32_t first_root, const uint32_t *size, std::chrono::steady_clock::time_point started, mc_live_info *out);
    int live_reach_tail(const LiveQuery &q, const uint32_t *scc, const uint32_t *size, uint32_t builds, const LiveCounters *d_lc, uint64_t strong_final,
                        hipStream_t stream, std::chrono::steady_clock::time_point started, mc_live_check_info *out);
};

// the one refusal of a bad query: live_query_error's words behind the call's name
inline int live_query_check(const LiveQuery &q, int npred) {
    const std::string why = live_query_error(q, npred);
    if (why.empty()) return MC_OK;
    set_error(std::string(q.call) + ": " + why);
    return MC_EBADCFG;
}

}  // namespace mc
