// violations.h — what TLC's -continue collects (MC_F_CONTINUE, mc_engine_violations), written once as MC_HD code: the device kernels
// (engine_violations.h) and the host (tests/_contshim, the counts the kernels must reproduce) run exactly this.
//
// A search that goes on past violations needs, per flagged BFS level, three things the single minimum key of DevCounters cannot say:
//   * which STORED states break an invariant, each once (viol_stored_bin: the status of the state itself, of Init, or of the
//     (parent, slot) pair that was first to find it — a lowering's status word carries the FIRST violated invariant only);
//   * which expanded states are deadlocked, and which violating successors lie OUTSIDE the model (never stored, counted per generation);
//   * whether anything FATAL happened in the level (a failed Assert, an evaluation error): the minimum key over those kinds alone —
//     the engine's key is a minimum over all kinds, so an invariant violator with a lower index hides an Assert failure of its level.
// The bins: 0 .. 31 = invariant index, VIOL_BIN_DEADLOCK, VIOL_BIN_FATAL.  Compiles without HIP (spec_*.h do too).
#pragma once
#include "mc_common.h"
#include "spec_registry.h"
#include "spec_gen.h"

namespace mc {

constexpr int VIOL_MAX_INV = 32;   // (a violation key has 5 bits for the invariant index)
constexpr int VIOL_BIN_DEADLOCK = 32, VIOL_BIN_FATAL = 33, VIOL_BINS = 34;

// lowerings that check their invariants when a state is EXPANDED (S::CHECK_ON_EXPAND; engine_kernels.h has the same trait for the kernels)
template <class S, class = void>
struct ViolChecksStored { static constexpr bool value = false; };
template <class S>
struct ViolChecksStored<S, decltype((void)S::CHECK_ON_EXPAND)> { static constexpr bool value = true; };

// INVARIANT indices of a model: the entries of mc_engine_violations, zero rows included
template <class S>
struct ViolModel;
template <> struct ViolModel<SpecAtomicAdd> { MC_HD static int ninv(const SpecAtomicAdd::Params &) { return 0; } };
template <> struct ViolModel<SpecPcalIntro> { MC_HD static int ninv(const SpecPcalIntro::Params &) { return 1; } };
template <int N> struct ViolModel<SpecRaft<N>> { MC_HD static int ninv(const RaftParams &) { return 2; } };
template <int N> struct ViolModel<SpecRaftPacked<N>> : ViolModel<SpecRaft<N>> {};
template <> struct ViolModel<SpecSsi> { MC_HD static int ninv(const SsiParams &) { return 8; } };   // seven invariants + the `find` predicate
// (the Paxos family's PROPERTY has an index of its own behind these — 1 / 4 — but no row: it is a property of a step, which no stored state
//  shows; viol_pair makes a pair that breaks it fatal, and the fatal entry names it)
template <> struct ViolModel<SpecPaxos> { MC_HD static int ninv(const PaxosParams &p) { return p.kind == 1 ? 1 : 4; } };
template <int MAXV> struct ViolModel<SpecVmT<MAXV>> { MC_HD static int ninv(const VmParams &p) { return p.ninv; } };
template <int MAXV> struct ViolModel<SpecVmCfgT<MAXV>> : ViolModel<SpecVmT<MAXV>> {};
template <class G> struct ViolModel<SpecGenT<G>> { MC_HD static int ninv(const VmParams &) { return G::NINV; } };

// What a (state, slot) pair of an EXPANDED state contributes.  One of:
enum : unsigned { VIOL_P_NONE = 0, VIOL_P_OUTSIDE = 1 /* bin = the invariant */, VIOL_P_FATAL = 2 /* bin = VIOL_BIN_FATAL, kind = VK_* of engine_kernels.h */ };
struct ViolPair { unsigned what, bin, kind, inv; bool flagged; /* flagged: the expand kernels set DevCounters::viol_key for it */ };
// (kinds as in engine_kernels.h: 1 invariant, 2 Assert, 4 evaluation error; the order of the tests is k_expand's)
template <class S>
MC_HD ViolPair viol_pair(unsigned st) {
    ViolPair r{VIOL_P_NONE, 0u, 0u, 0u, false};
    if (!(st & ST_ENABLED) || (st & ST_OVERFLOW)) return r;   // (an overflow is a DEV_E* error of the level: the search ends on it as ever)
    r.flagged = (st & (ST_ASSERT | ST_SPECERR | ST_INVARIANT)) != 0;
    if (st & ST_ASSERT) { r.what = VIOL_P_FATAL; r.bin = VIOL_BIN_FATAL; r.kind = 2u; return r; }
    if (st & ST_SPECERR) { r.what = VIOL_P_FATAL; r.bin = VIOL_BIN_FATAL; r.kind = 4u; return r; }
    if (!(st & ST_INVARIANT)) return r;
    r.bin = r.inv = (st >> 8) & 31u;
    r.kind = 1u;
    if (st & ST_OUT_OF_MODEL) { r.what = VIOL_P_OUTSIDE; return r; }
    // an in-model successor flagged by the PAIR of a lowering that checks stored states: a property of the step (Paxos' PROPERTY), which
    // no stored state shows — fatal, so that it is never dropped.  Everywhere else the stored pass counts the successor itself.
    if (ViolChecksStored<S>::value && !(st & ST_SELFLOOP)) { r.what = VIOL_P_FATAL; r.bin = VIOL_BIN_FATAL; }
    return r;
}
// ... with the model's number of invariant entries: an index BEHIND them is a property of the step (a compiled PlusCal program's
// `[][A]_v`), as Paxos' is — fatal whether or not the successor is new, in the model, or the expanded state itself, so
// that the search ends at the end of the level and the fatal entry, the last one, names it.  (A lowering that checks stored states keeps
// the rule above.)
template <class S>
MC_HD ViolPair viol_pair(unsigned st, int ninv) {
    ViolPair r = viol_pair<S>(st);
    if (!ViolChecksStored<S>::value && r.kind == 1u && (int)r.inv >= ninv) { r.what = VIOL_P_FATAL; r.bin = VIOL_BIN_FATAL; }
    return r;
}
// does the pair end the search at the end of its level?  (TLC treats a failed Assert and an evaluation error as fatal under -continue too)
MC_HD bool viol_ends_search(const ViolPair &r) { return r.what == VIOL_P_FATAL; }
// the column of the (states | outside) table a pair bumps in its bin, -1 = neither: a successor outside the model is not a stored state
MC_HD int viol_pair_column(const ViolPair &r) { return r.what == VIOL_P_OUTSIDE ? 1 : -1; }
// deadlock: an expanded state without an enabled slot
MC_HD bool viol_deadlocked(unsigned enabled_pairs, bool check_deadlock) { return check_deadlock && enabled_pairs == 0; }

// The invariant a STORED state is listed under, or -1.  self = the state's own row; has_parent = its trace record names a parent;
// own() -> the status of the state itself (lowerings that check stored states: S::parent_status / parent_status_step on the loaded row);
// ev() -> the status of S::eval on the (parent row, slot) pair that was first to find it.  The caller loads the rows: the device from the
// arena, the host from its store.
template <class S, class Ref, class Own, class Ev>
MC_HD int viol_stored_bin(const typename S::Params &prm, Ref self, bool has_parent, Own &&own, Ev &&ev) {
    unsigned st;
    if constexpr (ViolChecksStored<S>::value) { (void)prm; (void)self; (void)has_parent; (void)ev; st = own(); }
    else {
        (void)own;
        if (!has_parent) st = S::init_status(prm, self);        // an initial state
        else st = ev();
    }
    if (!(st & ST_INVARIANT) || (st & (ST_ASSERT | ST_SPECERR | ST_OUT_OF_MODEL))) return -1;
    return (int)((st >> 8) & 31u);
}
// ... with the model's number of invariant entries: no stored state is listed under the index of a property of a step (the pair that
// found it broke the property; the state itself breaks nothing)
template <class S, class Ref, class Own, class Ev>
MC_HD int viol_stored_bin(const typename S::Params &prm, Ref self, bool has_parent, int ninv, Own &&own, Ev &&ev) {
    const int bin = viol_stored_bin<S>(prm, self, has_parent, own, ev);
    return !ViolChecksStored<S>::value && bin >= ninv ? -1 : bin;
}

}  // namespace mc
