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
//   * strong fairness of whole processes (`fair+`): the refinement further down, DESIGN section 19.
//   * fairness label by label (`+` / `-` labels): units and conjuncts, at the end of this file, DESIGN section 21.
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
template <int MAXV> struct SpecVmCfgT;   // (spec_vm_cfg.h: the interpreter with the cfg's ACTION_CONSTRAINTs / VIEW — the same slots and processes)
template <int MAXV>
struct LiveProc<SpecVmCfgT<MAXV>> : LiveProc<SpecVmT<MAXV>> {};
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


// ---------------------------------------------------------------------------------------------------------------------------------------
// <>Q, []<>Q, <>[]P and P ~> Q (mc_engine_liveness_check): the same rule over the subgraph G[M] induced by a mask.
// A check is a triple of state sets, each a function of the state's predicate bits (bit k = predicate k; k_live_pred<S>) and of whether
// the state is initial:
//
//     kind                 M (a violating suffix stays in)   S (it may be entered at)     T (a state of it must recur)
//     LIVE_LEADS_TO  P~>Q  ~Q                                P /\ ~Q                      all
//     LIVE_INF_OFTEN []<>Q ~Q                                ~Q                           all
//     LIVE_EVENTUALLY <>Q  ~Q                                initial states with ~Q       all
//     LIVE_STABLE    <>[]P all                               all                          ~P
//
//   violated  iff  some strongly connected component C of G[M] (one-state components included) is fair, holds a T state and is
//   reachable along edges of G[M] from an S state that is itself in M.  taken(C) counts edges with both ends in C; en(s, p) — and so
//   disabled(C) — is taken in the FULL graph: an edge that leaves M still makes its process enabled.  That is live_state over the
//   component ids of G[M], in which every state outside M is a component of its own: scc[dst] == scc[self] never holds across the mask.
//
//   * LivePred<S>: the state predicates of a compiled program, evaluated on a loaded row.
//   * live_in_mask / live_in_start / live_in_target: the three sets.  live_own_component: which states the component search leaves out.
//     live_state_masked (then live_merge, as above, with "is a T state" in the Done flag's place) and live_violates_masked: the rule.
//     live_passable, live_reach_step: the reach pass.
constexpr int LIVE_LEADS_TO = 0, LIVE_INF_OFTEN = 1, LIVE_EVENTUALLY = 2, LIVE_STABLE = 3;
constexpr int LIVE_MAX_PREDS = 32;
constexpr uint32_t LIVE_FAR = 0xffffffffu;   // dist[] of a state from which no violating component is reached inside M

struct LiveCheck { int kind, p, q; };        // p / q: predicate indices, -1 = none

// what the host keeps about the predicates of a compiled program (defined in pcal_compile.cpp, beside vm_format): their number, with
// entries[k] = where predicate k's code starts in the image (at most cap of them); predicate k's text
int vm_live_preds(const void *host, int *entries, int cap);
const char *vm_live_pred_text(const void *host, int k);

// where the predicates' code is: entry[k] is the interpreter's code offset; generated code numbers them after its invariants
struct LivePredTab { int n; int entry[LIVE_MAX_PREDS]; };

template <class S>
struct LivePred {
    static constexpr bool HAS = false;
    MC_HD static int eval(const typename S::Params &, typename S::Local &, const LivePredTab &, int, int32_t &) { return 0; }
};
// eval: 1 = evaluated (res), 0 = an evaluation error inside the predicate
template <int MAXV>
struct LivePred<SpecVmT<MAXV>> {
    static constexpr bool HAS = true;
    MC_HD static int eval(const VmParams &p, typename SpecVmT<MAXV>::Local &l, const LivePredTab &tab, int k, int32_t &res) {
        int aux;
        return SpecVmT<MAXV>::run(p, tab.entry[k], 0, 0, 0, l.v, res, aux) == SpecVmT<MAXV>::R_OK;
    }
};
template <int MAXV>
struct LivePred<SpecVmCfgT<MAXV>> : LivePred<SpecVmT<MAXV>> {};
template <class G>
struct LivePred<SpecGenT<G>> {
    static constexpr bool HAS = true;
    MC_HD static int eval(const VmParams &, typename SpecGenT<G>::Local &l, const LivePredTab &, int k, int32_t &res) {
        return G::run_inv(G::NINV + G::NCON + k, l.v, res) == SpecGenT<G>::R_OK;
    }
};

MC_HD bool live_bit(uint32_t bits, int k) { return k >= 0 && (bits >> k & 1u); }
MC_HD bool live_in_mask(const LiveCheck &c, uint32_t bits) {
    return c.kind == LIVE_STABLE || !live_bit(bits, c.q);
}
MC_HD bool live_in_start(const LiveCheck &c, uint32_t bits, bool initial) {
    if (!live_in_mask(c, bits)) return false;   // (the S state itself must be in M)
    if (c.kind == LIVE_LEADS_TO) return live_bit(bits, c.p);
    if (c.kind == LIVE_EVENTUALLY) return initial;
    return true;
}
MC_HD bool live_in_target(const LiveCheck &c, uint32_t bits) {
    return c.kind == LIVE_STABLE ? !live_bit(bits, c.p) : true;
}
// the components of G[M]: a state outside M takes no part in the search, it is a component of its own
MC_HD bool live_own_component(const LiveCheck &c, uint32_t bits) {
    return !live_in_mask(c, bits);
}
// live_state for a state of M: *en from the whole row, *taken from the edges that stay in the state's component of G[M].  in_m(d): is
// state d in M; scc: the component ids of G[M].
template <class InM>
MC_HD void live_state_masked(uint32_t self, const uint32_t *dst, const int8_t *proc, uint64_t n, const uint32_t *scc, InM &&in_m, uint64_t *en, uint64_t *taken) {
    uint64_t en_ = 0, tk_ = 0;
    const uint32_t mine = scc[self];
    for (uint64_t k = 0; k < n; ++k) {
        const int p = proc[k];
        if (!live_real_step(p, self, dst[k])) continue;
        en_ |= 1ull << p;   // (the FULL graph's: an edge that leaves M still makes its process enabled)
        if (in_m(dst[k]) && scc[dst[k]] == mine) tk_ |= 1ull << p;
    }
    *en = en_;
    *taken = tk_;
}
// the component of G[M] with these unions over its states: a weakly fair suffix that stays in M and passes a T state for ever?
MC_HD bool live_violates_masked(uint64_t all, uint64_t fair, uint64_t taken, uint64_t disabled, bool has_target, uint32_t size) {
    return size >= 1 && has_target && live_fair(all, fair, taken, disabled);
}
// may a path from an S state to a violating component pass this state?  Only inside M.
MC_HD bool live_passable(const LiveCheck &c, uint32_t bits) {
    return live_in_mask(c, bits);
}
// The reach pass: dist[v] = 0 for the states of the violating components, else 1 + the least dist among the successors inside M
// (LIVE_FAR: none reaches one).  One update of a passable state `self` from its row; returns the new value (never larger than `mine`).
// in_m(d): is state d passable.  The fixed point is the length of the shortest path inside M to a violating component: unique, whatever
// the order of the updates.
template <class InM>
MC_HD uint32_t live_reach_step(uint32_t self, uint32_t mine, const uint32_t *dst, uint64_t n, const uint32_t *dist, InM &&in_m) {
    uint32_t best = mine;
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t d = dst[k];
        if (d == self || !in_m(d)) continue;
        const uint32_t dd = dist[d];
        if (dd != LIVE_FAR && dd + 1 < best) best = dd + 1;
    }
    return best;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Strong fairness of whole processes (`fair+ process`; mc_engine_liveness_strong / mc_engine_liveness_check_strong).
// Fair is split into W (weak) and F (strong), disjoint.  For a set X of M that is one state or strongly connected by its own edges:
//
//   enabled(X)    { p : en(s, p) for some s in X }                         (en in the FULL graph, as disabled(X))
//   X is fair     iff  W \subseteq taken(X) \cup disabled(X)  and  F \cap enabled(X) \subseteq taken(X)
//                 — a strongly fair process is taken inside X or disabled in EVERY state of X
//   violated      iff  some fair X holds a T state and is reachable inside M from an S state of M
//
// A component of G[M] need not be fair for a subset of it to be, so the components are refined (a Streett-style emptiness check).
// Every state of M starts open; a round finds the components of the subgraph induced by the open states and classifies each:
//
//   LIVE_CLOSE     no T state, or some p of W neither taken in C nor disabled somewhere in C: no subset of C is fair and holds a T state
//                  the first way, and every subset inherits the second defect — all of C is closed
//   LIVE_BLOCKED   B = F \cap enabled(C) \ taken(C) is not empty: the states s of C with en(s) \cap B # {} are closed, the rest stays open
//   LIVE_FINAL     else: C is fair, final and violating
//
//   every fair X survives inside one final component: X is strongly connected, so it lies in one component C of each round it is open in;
//   taken(X) \subseteq taken(C) and disabled(X) \subseteq disabled(C), so C is not weakly unfair, and it holds X's T state; a p of B is
//   not taken in C, so not in X, so — X being fair — it is enabled in no state of X: the states closed are none of X's.  X stays open
//   whole until its component is final.
//   a final component's closed walk is a fair suffix: C is one state or strongly connected inside the open states, so a closed walk
//   passes every state and every internal edge of C; every p of W is taken on it or disabled in a state of it; every p of F that is
//   enabled in a state of C is taken on it (B = {}), and the others are disabled along all of it.
//   A process of B is disabled in every state that survives, so it is in no later enabled(C'): at most popcount(F \cap all) rounds
//   block, and one more ends.  With F = {} the first round is the weak rule exactly.
//
//   * live_enabled_in: en of one state.  live_blockers: B.  live_classify: the three cases.  live_fair_strong / live_violates_strong:
//     the rule for one set.  live_closes_state: does a blocked component's state leave.  live_strong_rounds: the bound.
constexpr int LIVE_CLOSE = 0, LIVE_BLOCKED = 1, LIVE_FINAL = 2;
constexpr uint8_t LIVE_ST_CLOSED = 0, LIVE_ST_OPEN = 1, LIVE_ST_FINAL = 2;   // a state during the refinement

// the processes enabled in a state: the whole row's, in the full graph — never those of the open subgraph alone
MC_HD uint64_t live_enabled_in(uint32_t self, const uint32_t *dst, const int8_t *proc, uint64_t n, const uint32_t *scc) {
    uint64_t en = 0, tk = 0;   // (tk: the steps that stay in the state's component of the open subgraph — not what closes a state)
    live_state_masked(self, dst, proc, n, scc, [](uint32_t) { return true; }, &en, &tk);
    return en;
}
// the strongly fair processes that keep the component from being fair: enabled somewhere in it, taken nowhere inside it
MC_HD uint64_t live_blockers(uint64_t all, uint64_t strong, uint64_t enabled, uint64_t taken) {
    return strong & all & enabled & ~taken;
}
MC_HD bool live_fair_strong(uint64_t all, uint64_t weak, uint64_t strong, uint64_t taken, uint64_t disabled, uint64_t enabled) {
    return live_fair(all, weak, taken, disabled) && live_blockers(all, strong, enabled, taken) == 0;
}
MC_HD int live_classify(uint64_t all, uint64_t weak, uint64_t strong, uint64_t taken, uint64_t disabled, uint64_t enabled, bool has_target, uint32_t size) {
    if (!live_violates_masked(all, weak, taken, disabled, has_target, size)) return LIVE_CLOSE;
    return live_blockers(all, strong, enabled, taken) ? LIVE_BLOCKED : LIVE_FINAL;
}
MC_HD bool live_violates_strong(uint64_t all, uint64_t weak, uint64_t strong, uint64_t taken, uint64_t disabled, uint64_t enabled, bool has_target, uint32_t size) {
    return live_classify(all, weak, strong, taken, disabled, enabled, has_target, size) == LIVE_FINAL;
}
// a state of a blocked component, with its own en mask: it is closed iff a blocker is enabled in it
MC_HD bool live_closes_state(uint64_t blockers, uint64_t en) {
    return (en & blockers) != 0;
}
// what an open state becomes once its component is classified
MC_HD uint8_t live_refine_state(int cls, uint64_t blockers, uint64_t en) {
    if (cls == LIVE_FINAL) return LIVE_ST_FINAL;
    if (cls == LIVE_BLOCKED && !live_closes_state(blockers, en)) return LIVE_ST_OPEN;
    return LIVE_ST_CLOSED;
}
// the rounds a refinement may take: every blocking round disables a strongly fair process for good
MC_HD uint32_t live_strong_rounds(uint64_t all, uint64_t strong) {
    uint32_t k = 1;
    for (uint64_t f = strong & all; f; f &= f - 1) ++k;
    return k;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Fairness label by label (mc_engine_liveness_units / mc_engine_liveness_check_units).  Two notions replace "process":
//
//   unit       the class of an edge (unit[] in proc[]'s place, LIVE_TERM as before, at most LIVE_MAX_UNITS): a function of the instance
//              that steps and of the label at pc[self] in the SOURCE state
//   conjunct   one WF_vars / SF_vars conjunct of the translation's Spec, at most LIVE_MAX_CONJ: a set of units of one instance.
//              of_unit[u] = the conjuncts unit u belongs to — two for a `+` label of a weakly fair process (the process's WF, its own
//              SF), none for a `-` label or a label of an unfair process
//
// Every mask of the rule — en, taken, disabled, enabled, the blockers, weak / strong, all — is then a mask of CONJUNCTS: an edge
// contributes of_unit[u] where it contributed 1ull << p, and the functions above that take masks alone (live_merge, live_fair,
// live_classify, live_refine_state, live_strong_rounds, ...) are used as they are.  With of_unit[u] = 1ull << u the three functions
// below are live_state, live_state_masked and live_enabled_in.
constexpr int LIVE_MAX_UNITS = 127, LIVE_MAX_CONJ = 64;
constexpr int LIVE_UNIT_TAB = 128;   // entries of an of_unit[] table: every int8_t unit >= 0 indexes inside it

// the conjuncts an edge of unit u counts for
MC_HD uint64_t live_conjuncts(const uint64_t *of_unit, int u) {
    return u >= 0 ? of_unit[u] : 0;
}
MC_HD void live_state_units(uint32_t self, const uint32_t *dst, const int8_t *unit, uint64_t n, const uint32_t *scc, const uint64_t *of_unit, uint64_t *en,
                            uint64_t *taken, bool *done) {
    uint64_t e = 0, t = 0;
    bool d = false;
    const uint32_t mine = scc[self];
    for (uint64_t k = 0; k < n; ++k) {
        const int u = unit[k];
        if (u == LIVE_TERM) d = true;
        if (!live_real_step(u, self, dst[k])) continue;
        const uint64_t c = live_conjuncts(of_unit, u);
        e |= c;
        if (scc[dst[k]] == mine) t |= c;
    }
    *en = e;
    *taken = t;
    *done = d;
}
template <class InM>
MC_HD void live_state_masked_units(uint32_t self, const uint32_t *dst, const int8_t *unit, uint64_t n, const uint32_t *scc, const uint64_t *of_unit, InM &&in_m,
                                   uint64_t *en, uint64_t *taken) {
    uint64_t e = 0, t = 0;
    const uint32_t mine = scc[self];
    for (uint64_t k = 0; k < n; ++k) {
        const int u = unit[k];
        if (!live_real_step(u, self, dst[k])) continue;
        const uint64_t c = live_conjuncts(of_unit, u);
        e |= c;   // (the FULL graph's, as in live_state_masked)
        if (in_m(dst[k]) && scc[dst[k]] == mine) t |= c;
    }
    *en = e;
    *taken = t;
}
// the conjuncts enabled in a state: the whole row's, in the full graph
MC_HD uint64_t live_enabled_in_units(uint32_t self, const uint32_t *dst, const int8_t *unit, uint64_t n, const uint32_t *scc, const uint64_t *of_unit) {
    uint64_t e = 0, t = 0;
    live_state_masked_units(self, dst, unit, n, scc, of_unit, [](uint32_t) { return true; }, &e, &t);
    return e;
}
// LiveLabel<S>: the label instance `inst` stands at (the pc cell of the row the walk has loaded — the lowering's own load, never the
// raw words of a packed row), -1 where the lowering has no processes.  LiveUnitTab: unit[inst * nlabels + label] in device memory;
// live_unit_of: the unit of an edge taken by `inst` from a state where it stands at `label`; a pair the table does not hold is the
// instance's own unit (units 0 .. ninst - 1), never LIVE_TERM: that would read the edge as the terminating disjunct's.
template <class S>
struct LiveLabel {
    MC_HD static int of(const typename S::Params &, const typename S::Local &, int) { return -1; }
};
template <int MAXV>
struct LiveLabel<SpecVmT<MAXV>> {
    MC_HD static int of(const VmParams &p, const typename SpecVmT<MAXV>::Local &l, int inst) { return inst >= 0 && inst < p.ninst ? l.v[p.pc_base + inst] : -1; }
};
template <int MAXV>
struct LiveLabel<SpecVmCfgT<MAXV>> : LiveLabel<SpecVmT<MAXV>> {};
template <class G>
struct LiveLabel<SpecGenT<G>> {
    template <int I>
    MC_HD static int chain(const typename SpecGenT<G>::Local &l, int inst) {
        if constexpr (I < G::NINST) return inst == I ? (int)G::template pc_of<I>(l.v) : chain<I + 1>(l, inst);
        else return -1;
    }
    MC_HD static int of(const VmParams &, const typename SpecGenT<G>::Local &l, int inst) { return chain<0>(l, inst); }
};
struct LiveUnitTab { int ninst, nlabels; const int8_t *unit; };
MC_HD int live_unit_of(const LiveUnitTab &t, int inst, int label) {
    if (inst < 0 || inst >= t.ninst || inst > LIVE_MAX_UNITS - 1) return LIVE_TERM;
    return label >= 0 && label < t.nlabels ? t.unit[inst * t.nlabels + label] : inst;   // (a label the table does not know: the instance's own unit)
}
// the unit of the edge a (state, slot) pair contributes: the slot's instance and the label it stands at in `src`, the loaded row of the
// SOURCE state; LIVE_TERM for the terminating disjunct alone
template <class S>
MC_HD int live_edge_unit(const typename S::Params &prm, const typename S::Local &src, const LiveUnitTab &tab, int slot) {
    const int inst = LiveProc<S>::of(prm, slot);
    return inst == LIVE_TERM ? LIVE_TERM : live_unit_of(tab, inst, LiveLabel<S>::of(prm, src, inst));
}
// what the host keeps about the units of a compiled program (defined in pcal_compile.cpp, beside vm_live_preds): the number of units,
// with *ninst / *nlabels the table's shape and unit_out[inst * nlabels + label] filled when cap holds it (cap 0: the shape alone)
int vm_live_units(const void *host, int *ninst, int *nlabels, int8_t *unit_out, int cap);
// every conjunct of a table with nconj conjuncts
MC_HD uint64_t live_all_conjuncts(int nconj) {
    return nconj >= 64 ? ~0ull : (1ull << nconj) - 1;
}

}  // namespace mc
