// tests/_sideshim/spec_table.h — a TEST-ONLY lowering whose rows ARE the test case: everything the side passes ask of a lowering S
// (engine_graph.h, engine_coverage.h, engine_violations.h; on the host graph.h, coverage.h, violations.h, liveness.h) is read from the
// row, so a test writes any graph and any status word by hand.  It satisfies the concept of SpecAtomicAdd (spec_pluscal.h) as far as
// those passes use it: Params, Local, words, load, nslots, eval, fp_of, init_status, parent_status.  Compiles without HIP.
//
// A row has 4 + 2 * Params::max_slots 64-bit words:
//   word 0          the state's own key, used as its fingerprint VERBATIM (fp_of = word 0): a test picks home buckets
//                   ((key & 0xffffffff) * nbuckets >> 32) and builds chains, full buckets and wrap-arounds itself
//   word 1          bits 0..15   nslots (clamped to Params::max_slots: no row can send a walk past its own words)
//                   bits 16..31  the state's OWN status word (parent_status: what a lowering that checks stored states finds in it)
//                   bits 32..47  its init_status (what Init's check said of it)
//   word 2          bits 0..31   the predicate bits: bit k = predicate k holds;  bits 32..63: bit 32 + k = predicate k FAILS to evaluate
//   word 3          8 bits per process instance (instances 0 .. 7): the label the instance stands at (LiveLabel)
//   word 4 + 2k     slot k: bits 0..31 the status S::eval returns (ST_* flags, the invariant index in bits 8..12);
//                           bits 32..63 the action id of the pair, a signed 32-bit number (CovAction::of)
//   word 5 + 2k     slot k: the 64-bit key S::eval leaves in f
//
// Two variants over the same rows, because k_viol_stored and viol_pair branch on the trait at compile time:
//   SpecTab         checks on generation (no CHECK_ON_EXPAND);
//   SpecTabStored   declares CHECK_ON_EXPAND: ChecksOnExpand / ViolChecksStored are true.
// Processes: slot k is taken by instance k / maxch; slots at or past ninst * maxch are the terminating disjunct's (LIVE_TERM).
#pragma once
#include "coverage.h"
#include "liveness.h"
#include "violations.h"

namespace mc {

struct SpecTabParams { int max_slots, nbins, ninst, maxch; };
constexpr int SPECTAB_HEAD = 4, SPECTAB_MAX_SLOTS = 64;

struct SpecTabBase {
    using Params = SpecTabParams;
    struct Local { uint64_t w1, w2, w3; };
    static constexpr int MAX_WORDS = SPECTAB_HEAD + 2 * SPECTAB_MAX_SLOTS;
    MC_HD static int words(const Params &p) { return SPECTAB_HEAD + 2 * p.max_slots; }
    MC_HD static int max_slots(const Params &p) { return p.max_slots; }
    MC_HD static uint64_t fp_of(const Params &, CWordRef s) { return s.get(0); }
    MC_HD static unsigned init_status(const Params &, CWordRef s) { return (unsigned)(s.get(1) >> 32) & 0xffffu; }
    MC_HD static void load(const Params &, CWordRef s, Local &l) { l.w1 = s.get(1); l.w2 = s.get(2); l.w3 = s.get(3); }
    MC_HD static int nslots(const Params &p, const Local &l) {
        const int n = (int)(l.w1 & 0xffffu);
        return n < p.max_slots ? n : p.max_slots;
    }
    MC_HD static unsigned parent_status(const Params &, const Local &l, CWordRef) { return (unsigned)(l.w1 >> 16) & 0xffffu; }
    MC_HD static bool in_row(const Params &p, int slot) { return slot >= 0 && slot < p.max_slots; }
    MC_HD static unsigned eval(const Params &p, const Local &, CWordRef s, int slot, uint64_t &fp) {
        if (!in_row(p, slot)) return 0;
        fp = s.get(SPECTAB_HEAD + 2 * slot + 1);
        return (unsigned)(s.get(SPECTAB_HEAD + 2 * slot) & 0xffffffffull);
    }
    MC_HD static int action_id(const Params &p, CWordRef s, int slot) {
        return in_row(p, slot) ? (int)(int32_t)(uint32_t)(s.get(SPECTAB_HEAD + 2 * slot) >> 32) : -1;
    }
};
struct SpecTab : SpecTabBase {};
struct SpecTabStored : SpecTabBase { static constexpr int CHECK_ON_EXPAND = 1; };

struct SpecTabCov {
    static constexpr bool BY_SLOT = false;
    MC_HD static int nbins(const SpecTabParams &p) { return p.nbins; }
    MC_HD static bool listed(const SpecTabParams &p, int a) { return a >= 0 && a + 1 < p.nbins; }
    MC_HD static int of(const SpecTabParams &p, const SpecTabBase::Local &, CWordRef s, int slot) { return SpecTabBase::action_id(p, s, slot); }
};
template <> struct CovAction<SpecTab> : SpecTabCov {};
template <> struct CovAction<SpecTabStored> : SpecTabCov {};

struct SpecTabProc {
    static constexpr bool HAS = true;
    MC_HD static int count(const SpecTabParams &p) { return p.ninst; }
    MC_HD static int of(const SpecTabParams &p, int slot) { return slot >= p.ninst * p.maxch ? LIVE_TERM : slot / p.maxch; }
};
template <> struct LiveProc<SpecTab> : SpecTabProc {};
template <> struct LiveProc<SpecTabStored> : SpecTabProc {};

struct SpecTabLabel {
    MC_HD static int of(const SpecTabParams &p, const SpecTabBase::Local &l, int inst) {
        return inst >= 0 && inst < p.ninst && inst < 8 ? (int)((l.w3 >> (8 * inst)) & 0xffu) : -1;
    }
};
template <> struct LiveLabel<SpecTab> : SpecTabLabel {};
template <> struct LiveLabel<SpecTabStored> : SpecTabLabel {};

struct SpecTabPred {   // eval: 1 = evaluated (res), 0 = an evaluation error inside the predicate
    static constexpr bool HAS = true;
    MC_HD static int eval(const SpecTabParams &, SpecTabBase::Local &l, const LivePredTab &, int k, int32_t &res) {
        if (l.w2 >> (32 + k) & 1u) return 0;
        res = (int32_t)(l.w2 >> k & 1u);
        return 1;
    }
};
template <> struct LivePred<SpecTab> : SpecTabPred {};
template <> struct LivePred<SpecTabStored> : SpecTabPred {};

template <> struct ViolModel<SpecTab> { MC_HD static int ninv(const SpecTabParams &) { return VIOL_MAX_INV; } };
template <> struct ViolModel<SpecTabStored> : ViolModel<SpecTab> {};

}  // namespace mc
