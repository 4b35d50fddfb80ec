// liveness.h — the rule by which `Termination` of a weakly fair PlusCal algorithm is decided on the state graph (mc_engine_liveness),
// written once as MC_HD code: the device kernels (engine_live.h) and the host (the counterexample builder of engine.hip;
// tests/_liveshim, a g++ build that the host tests compare with an independent reference and mutate) run exactly this.  DESIGN section 16
// has the argument; in short, for  Spec == Init /\ [][Next]_vars /\ \A p \in Fair : WF_vars(proc_p)  over the COMPLETE reachable graph:
//
//   en(s, p)      s has an out-edge taken by process instance p to a DIFFERENT state (ENABLED <proc_p>_vars)
//   taken(C)      { p : some edge u -> v of p with u # v and u, v in the strongly connected component C }
//   disabled(C)   { p : some s in C with ~en(s, p) }
//   C is fair     iff  Fair \subseteq taken(C) \cup disabled(C)
//   Termination is violated  iff  some fair C — one-state components without an internal edge included — holds no Done state
//
//   * LiveProc<S>: which process instance takes the edge of a (state, slot) pair — slot / maxch for the two compiled-program
//     lowerings, LIVE_TERM for the terminating disjunct.  Other lowerings have no processes: LiveProc<S>::HAS is false.
//   * live_real_step, live_state, live_merge, live_fair, live_violates: the rule over CSR rows, per-edge processes and component ids.
// Compiles without HIP.
#pragma once
#include "graph.h"

namespace mc {

constexpr int LIVE_TERM = -1;   // proc[] of an edge of the terminating disjunct ((\A self: pc[self] = "Done") /\ UNCHANGED vars)
constexpr int LIVE_MAX_PROCS = 64;

template <class S>
struct LiveProc {
    static constexpr bool HAS = false;
    MC_HD static int count(const typename S::Params &) { return 0; }
    MC_HD static int of(const typename S::Params &, int) { return LIVE_TERM; }
};
template <int MAXV>
struct LiveProc<SpecVmT<MAXV>> {
    static constexpr bool HAS = true;
    MC_HD static int count(const VmParams &p) { return p.ninst; }
    MC_HD static int of(const VmParams &p, int slot) { return slot >= p.ninst * p.maxch ? LIVE_TERM : slot / p.maxch; }
};
template <class G>
struct LiveProc<SpecGenT<G>> {
    static constexpr bool HAS = true;
    MC_HD static int count(const VmParams &) { return G::NINST; }
    MC_HD static int of(const VmParams &, int slot) { return slot >= G::NINST * G::MAXCH ? LIVE_TERM : slot / G::MAXCH; }
};

// is the edge src -> dst, taken by `proc`, a step <proc_p>_vars?  An edge that ends where it starts changes no variable: it is a
// stuttering step, whoever takes it (a one-label `while TRUE do skip` produces one).
MC_HD bool live_real_step(int proc, uint32_t src, uint32_t dst) {
    return proc >= 0 && src != dst;
}

// One state's row: *en = the processes enabled in it, *taken = those with a real step that stays inside the state's component,
// *done = the terminating disjunct is enabled (a Done state).  scc: the component id of every state.
MC_HD void live_state(uint32_t self, const uint32_t *dst, const int8_t *proc, uint64_t n, const uint32_t *scc, uint64_t *en, uint64_t *taken, bool *done) {
    uint64_t e = 0, t = 0;
    bool d = false;
    const uint32_t mine = scc[self];
    for (uint64_t k = 0; k < n; ++k) {
        const int p = proc[k];
        if (p == LIVE_TERM) d = true;
        if (!live_real_step(p, self, dst[k])) continue;
        e |= 1ull << p;
        if (scc[dst[k]] == mine) t |= 1ull << p;
    }
    *en = e;
    *taken = t;
    *done = d;
}
// the processes (of `all`: one bit per instance) that are disabled in a state, given its en mask
MC_HD uint64_t live_disabled(uint64_t all, uint64_t en) {
    return all & ~en;
}
// a component's entry: the unions over its states, merged one state at a time (the device merges with atomicOr at scc[v])
struct LiveComp {
    uint64_t taken = 0, disabled = 0;
    bool done = false, first = true;
    uint32_t size = 0;
};
MC_HD void live_merge(LiveComp &c, uint64_t taken, uint64_t disabled, bool done) {
    c.taken |= taken;
    c.disabled = c.disabled | disabled;
    c.done = c.done || done;
    c.first = false;
    ++c.size;
}
// all: one bit per process instance of the program; fair: the weakly fair ones among them
MC_HD bool live_fair(uint64_t all, uint64_t fair, uint64_t taken, uint64_t disabled) {
    const uint64_t need = fair & all;
    return (need & ~(taken | disabled)) == 0;
}
// does the component hold a weakly fair behaviour suffix that never terminates?  One-state components count: without an internal edge
// the behaviour stutters there.  (Done states are absorbing: a component with one is that one state.)
MC_HD bool live_violates(uint64_t all, uint64_t fair, uint64_t taken, uint64_t disabled, bool has_done, uint32_t size) {
    return size >= 1 && !has_done && live_fair(all, fair, taken, disabled);
}

}  // namespace mc
