// state_graph.h — the state graph of a finished search (mc_engine_graph) and what is computed from its CSR arrays alone: the reads, the
// strongly connected components (mc_engine_scc), the fairness check (mc_engine_liveness) and its counterexample.  None of it depends on
// the lowering, so the host half (state_graph.hip) and the kernels (engine_live.h) are compiled once for the library; the engine of
// every lowering — the one of generated code, built at load time, included — fills the arrays with its own kernels (engine_graph.h:
// k_graph_index / k_graph_degree / k_graph_fill / k_live_proc) and calls in here.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tlamc.h"
#include "hip_owned.h"

namespace mc {

struct LiveCheck;      // liveness.h
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
        bool scc_built = false, checked = false;
        DevBuf<uint64_t> toff;      // [states + 1] rows of the transpose (self loops left out)
        DevBuf<uint32_t> tsrc;      // [edges that are no self loops] the sources
        DevBuf<uint32_t> scc;       // [states] the least arena index of the state's component
        DevBuf<uint32_t> size;      // [states] at a component's id: its number of states
        DevBuf<int8_t> proc;        // [edges] beside act: the process instance that takes the edge, LIVE_TERM for the terminating disjunct
        DevBuf<unsigned long long> taken, disabled;   // [states] at a component's id: the unions over its states
        DevBuf<unsigned> done;      // [states] at a component's id: it holds a Done state
        mc_scc_info sinfo{};
        mc_live_info linfo{};
        uint64_t fair = 0, strong = 0;   // of the last check: the weakly / strongly fair processes
        // what mc_engine_predicates / mc_engine_liveness_check add
        bool pred_built = false, proc_built = false;
        DevBuf<uint32_t> pred;      // [states] bit k = predicate k of the program's temporal properties holds in the state
        DevBuf<uint32_t> dist;      // [states] the reach pass of the last check
        struct Masked { int q; DevBuf<uint32_t> scc, size; };   // the components of the subgraph induced by ~predicate q: one build per mask
        std::vector<std::unique_ptr<Masked>> masks;
        // the last check, for the counterexample: -1 = Termination (mc_engine_liveness), else the kind of a property check
        int last_kind = -1, last_p = -1, last_q = -1;
        const Masked *last_mask = nullptr;     // its components (null: the full graph's)
        std::vector<uint32_t> descent;         // from the witness along falling dist to the first state of the component
        // what mc_engine_liveness_strong / mc_engine_liveness_check_strong add
        bool last_strong = false;              // the last check refined: its components are fscc's
        DevBuf<unsigned long long> enabled;    // [states] at a component's id: the processes enabled in some state of it
        DevBuf<uint8_t> open;                  // [states] LIVE_ST_*: closed, open or in a final component
        DevBuf<uint32_t> fscc, fsize;          // [states] the refined ids (a closed state: its own index) and, at an id, the size
        DevBuf<uint32_t> wscc, wsize;          // [states] the components of the open subgraph, rounds >= 2
        // what mc_engine_liveness_units / mc_engine_liveness_check_units add
        bool last_units = false;               // the last check read proc[] as units: fair / strong are masks of conjuncts
        bool unit_built = false;
        DevBuf<int8_t> unit;                   // [edges] beside proc: the edge's unit (k_live_unit<S>), LIVE_TERM for the terminating disjunct
        DevBuf<uint64_t> of_unit;              // [LIVE_UNIT_TAB] the conjuncts of every unit, as the kernels stage it
        std::vector<uint64_t> of_unit_host;    // the same, for the counterexample builder
        void release() {
            scc_built = checked = pred_built = proc_built = false;
            toff.reset(); tsrc.reset(); scc.reset(); size.reset(); proc.reset(); taken.reset(); disabled.reset(); done.reset();
            pred.reset(); dist.reset(); masks.clear(); descent.clear();
            enabled.reset(); open.reset(); fscc.reset(); fsize.reset(); wscc.reset(); wsize.reset();
            last_kind = -1; last_mask = nullptr; last_strong = false; strong = 0;
            last_units = unit_built = false; unit.reset(); of_unit.reset(); of_unit_host.clear();
        }
    } lv;
    void release() { built = false; offsets.reset(); dst.reset(); act.reset(); lv.release(); }

    // mc_engine_graph_read
    int read(uint64_t first, uint64_t count, uint64_t *offsets_out, uint32_t *dst_out, int32_t *action_out, size_t *nedges_inout);
    // mc_engine_scc on a built graph, mc_engine_scc_read
    int scc(hipStream_t stream, mc_scc_info *out);
    int scc_read(uint64_t first, uint64_t count, uint32_t *scc_out);
    // mc_engine_liveness once the components are found and the engine's k_live_proc<S> is enqueued on `stream` (lv.proc): the rule
    // over `all` process instances, `fair` of them weakly fair.  started: when the call began (mc_live_info.seconds).
    int live_check(uint64_t all, uint64_t fair, hipStream_t stream, std::chrono::steady_clock::time_point started, mc_live_info *out);
    // mc_engine_liveness_trace; level_start: the search's level table (arena index of each BFS level's first state)
    // mc_engine_predicates once the engine's k_live_pred<S> has filled lv.pred
    int pred_read(uint64_t first, uint64_t count, uint32_t *bits_out);
    // mc_engine_liveness_check once the components, lv.proc and lv.pred are there: kind / p / q as in mc_live_property (validated by
    // the caller against the program's predicates)
    int live_check_masked(uint64_t all, uint64_t fair, int kind, int p, int q, hipStream_t stream, std::chrono::steady_clock::time_point started,
                          mc_live_check_info *out);
    // mc_engine_liveness_strong (kind < 0: lout) / mc_engine_liveness_check_strong (cout), after the same preparation as the weak twins
    // of_unit (mc_engine_liveness_units / mc_engine_liveness_check_units): lv.unit is read in lv.proc's place, the masks are over conjuncts
    int live_check_strong(uint64_t all, uint64_t weak, uint64_t strong, int kind, int p, int q, hipStream_t stream,
                          std::chrono::steady_clock::time_point started, mc_live_info *lout, mc_live_check_info *cout, mc_live_strong_info *sout,
                          const uint64_t *of_unit = nullptr);
    int live_scc_read(uint64_t first, uint64_t count, uint32_t *scc_out);   // mc_engine_liveness_components
    int live_unit_read(uint64_t first, uint64_t count, int8_t *unit_out);   // mc_engine_liveness_edge_units
    int live_trace(const std::vector<uint64_t> &level_start, uint32_t *prefix_out, size_t *nprefix_inout, uint32_t *cycle_out, size_t *ncycle_inout);

private:
    int scc_build(uint64_t n, hipStream_t stream);
    // trim + colouring over the transpose that is there; mask: the predicate whose states are left out (a component of their own each), -1 = none
    // open: (rounds >= 2 of a strong check) only the states with LIVE_ST_OPEN there take part, in place of a predicate mask
    int scc_components(uint64_t n, hipStream_t stream, int mask_q, DevBuf<uint32_t> &scc_buf, DevBuf<uint32_t> &size_buf, mc_scc_info &info,
                       const uint8_t *open = nullptr);
    int live_mask_components(int kind, int q, hipStream_t stream, const Live::Masked **mask_out, uint32_t *builds);
    int live_reach_tail(const LiveCheck &ck, const uint32_t *scc, const uint32_t *size, const Live::Masked *mask, uint64_t fair, uint64_t strong,
                        bool is_strong, uint32_t builds, const LiveCounters *d_lc, uint64_t strong_final, hipStream_t stream,
                        std::chrono::steady_clock::time_point started, mc_live_check_info *out);
};

}  // namespace mc
