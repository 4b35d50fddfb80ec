// live_query.h — ONE description of a liveness check and ONE validation of it, host only: the six C entries (mc_engine_liveness,
// mc_engine_liveness_check and their _strong / _units twins) each fill a LiveQuery, and the engine (engine.hip), the graph passes
// (StateGraph::live_check, state_graph.hip) and the test drivers of those passes all refuse a bad one with live_query_error's words.
// Everything here is independent of the lowering and of the graph; what depends on them (a sharded engine, a search that did not
// finish, a program with more units than the table) is the engine's.  Compiles without HIP (tests/_queryshim).
#pragma once
#include <cstdint>
#include <string>

#include "../../include/tlamc.h"
#include "liveness.h"   // LIVE_*: the kinds and the bounds; live_all_conjuncts

namespace mc {

struct LiveQuery {
    const char *call;          // the C-ABI name of the call, for messages
    uint64_t all;              // every process instance there is — with `fu`: every conjunct (live_query_units sets it)
    uint64_t weak, strong;     // the weakly / strongly fair ones among them
    const mc_fair_units *fu;   // the table of a check label by label, null for a process-level check
    int kind, p, q;            // -1: Termination, else LIVE_LEADS_TO .. LIVE_STABLE over the predicates p / q
    bool refine;               // false: the single pass of the two weak entries; true: the refinement rounds (strong and unit entries)
    bool term() const { return kind == -1; }
    bool need_p() const { return kind == LIVE_LEADS_TO || kind == LIVE_STABLE; }
    bool need_q() const { return kind >= 0 && kind != LIVE_STABLE; }
};

// the query of a check label by label: the masks are the table's, `all` its conjuncts (none when nconj is out of range: refused below)
inline LiveQuery live_query_units(const char *call, const mc_fair_units *fu, int kind, int p, int q) {
    const uint64_t all = fu->nconj >= 0 && fu->nconj <= LIVE_MAX_CONJ ? live_all_conjuncts(fu->nconj) : 0;
    return LiveQuery{call, all, fu->weak_mask, fu->strong_mask, fu, kind, p, q, true};
}

inline std::string live_unknown_kind(int kind) { return "unknown kind " + std::to_string(kind); }

// "" for a good query, else why it is refused (the caller puts "<call>: " in front); npred: the predicates the program has
inline std::string live_query_error(const LiveQuery &q, int npred) {
    if (const mc_fair_units *fu = q.fu) {
        if (fu->nunits < 0 || fu->nunits > LIVE_MAX_UNITS) return std::to_string(fu->nunits) + " units (at most 127)";
        if (fu->nconj < 0 || fu->nconj > LIVE_MAX_CONJ) return std::to_string(fu->nconj) + " conjuncts (at most 64)";
    }
    const uint64_t all = q.fu ? live_all_conjuncts(q.fu->nconj) : q.all;
    if ((q.weak | q.strong) & ~all)
        return q.fu ? "a fairness mask names a conjunct beyond nconj"
                    : std::string(q.refine ? "a" : "the") + " fairness mask names a process instance the program does not have";
    if (q.weak & q.strong)
        return std::string("the weak and the strong mask overlap ") + (q.fu ? "(a conjunct is WF or SF)" : "(a strongly fair process is weakly fair already)");
    if (const mc_fair_units *fu = q.fu)
        for (int u = 0; u < LIVE_UNIT_TAB; ++u)
            if (fu->of_unit[u] & (u < fu->nunits ? ~all : ~0ull))
                return "of_unit[" + std::to_string(u) + "] names " + (u < fu->nunits ? "a conjunct beyond nconj" : "conjuncts for a unit beyond nunits");
    if (q.term()) return {};
    if (q.kind < LIVE_LEADS_TO || q.kind > LIVE_STABLE) return live_unknown_kind(q.kind);
    if ((q.need_p() && (q.p < 0 || q.p >= npred)) || (q.need_q() && (q.q < 0 || q.q >= npred)) || npred > LIVE_MAX_PREDS)
        return "a predicate index the program does not have (it has " + std::to_string(npred) + " predicates)";
    return {};
}

// a p or q the kind does not need becomes -1: what the passes and the counterexample builder are handed
inline LiveQuery live_query_normalised(LiveQuery q) {
    if (!q.need_p()) q.p = -1;
    if (!q.need_q()) q.q = -1;
    return q;
}

}  // namespace mc
