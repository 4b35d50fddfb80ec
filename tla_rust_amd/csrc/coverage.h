// coverage.h — what TLC's -coverage counts (MC_F_COVERAGE, mc_engine_coverage), written once as MC_HD code: the device kernels
// (engine_coverage.h) and the host (tests/_covshim, the counts the kernels must reproduce) run exactly this.
//
//   * which (state, slot) pairs count: cov_counts(status) — every pair whose S::eval status has ST_ENABLED, whatever else it carries
//     (a failed Assert, an evaluation error, an out-of-model successor, a self loop): the pairs k_expand counts into
//     mc_result.generated;
//   * which action a pair belongs to, ON THE DEVICE: CovAction<S>, one small trait per lowering over what the lowering already has as
//     MC_HD code (S::action_of is host code in most of them).  The ids are mc_action_name's.
//
// CovAction<S>:
//   nbins(prm)                 bins of a histogram: bin 0 = Init (action id -1), bin a + 1 = action id a
//   listed(prm, a)             is action id a an action of THIS model (an entry of mc_engine_coverage)?  The Paxos lowering serves two
//                              modules with disjoint ids; "Done" is a label id of a compiled program but no action
//   BY_SLOT                    the action is a function of (prm, slot) alone — wave-uniform in a kernel whose lanes walk the slots together
//   of(prm, loc, s, slot)      the action id of the pair (state s, loaded into loc; slot)
// Compiles without HIP (spec_*.h do too).
#pragma once
#include "mc_common.h"
#include "spec_registry.h"
#include "spec_gen.h"

namespace mc {

constexpr int COV_MAX_BINS = 512;   // bins of the per-workgroup LDS histogram (2 KiB); an engine of a model with more actions refuses the flag

MC_HD bool cov_counts(unsigned st) { return (st & ST_ENABLED) != 0; }

template <class S>
struct CovAction;

template <>
struct CovAction<SpecAtomicAdd> {
    static constexpr bool BY_SLOT = true;
    MC_HD static int nbins(const SpecAtomicAdd::Params &) { return 3 + 1; }
    MC_HD static bool listed(const SpecAtomicAdd::Params &, int a) { return a >= 0 && a < 3; }
    template <class Ref>
    MC_HD static int of(const SpecAtomicAdd::Params &p, const SpecAtomicAdd::Local &, Ref, int slot) { return SpecAtomicAdd::action_of(p, nullptr, slot); }
};
template <>
struct CovAction<SpecPcalIntro> {
    static constexpr bool BY_SLOT = false;   // the label the slot's process stands at
    MC_HD static int nbins(const SpecPcalIntro::Params &) { return 5 + 1; }
    MC_HD static bool listed(const SpecPcalIntro::Params &, int a) { return a >= 0 && a < 5; }
    template <class Ref>
    MC_HD static int of(const SpecPcalIntro::Params &p, const SpecPcalIntro::Local &l, Ref, int slot) { return SpecPcalIntro::action_of(p, &l.w, slot); }
};
template <>
struct CovAction<SpecPaxos> {
    static constexpr bool BY_SLOT = true;
    MC_HD static int nbins(const PaxosParams &) { return 6 + 1; }
    MC_HD static bool listed(const PaxosParams &p, int a) { return p.kind == 1 ? (a >= 0 && a < 2) : (a >= 2 && a < 6); }   // Voting | Paxos
    template <class Ref>
    MC_HD static int of(const PaxosParams &p, const SpecPaxos::Local &, Ref, int slot) { return SpecPaxos::action_of(p, nullptr, slot); }
};
// raft, SSI: compute() yields the action of the pair it evaluates
template <int N>
struct CovAction<SpecRaft<N>> {
    using S = SpecRaft<N>;
    static constexpr bool BY_SLOT = false;   // (a message slot's action is the kind of the message in it)
    MC_HD static int nbins(const RaftParams &) { return 10 + 1; }
    MC_HD static bool listed(const RaftParams &, int a) { return a >= 0 && a < 10; }
    template <class Ref>
    MC_HD static int of(const RaftParams &p, const typename S::Local &l, Ref s, int slot) {
        typename S::Delta d;
        int action = -1;
        S::compute(p, l, s, slot, d, action);
        return action;
    }
};
template <int N>
struct CovAction<SpecRaftPacked<N>> : CovAction<SpecRaft<N>> {   // (spec_raft_packed.h: its compute() reads the stored row through the view)
    using S = SpecRaftPacked<N>;
    template <class Ref>
    MC_HD static int of(const RaftParams &p, const typename S::Local &l, Ref s, int slot) {
        typename S::Delta d;
        int action = -1;
        S::compute(p, l, s, slot, d, action);
        return action;
    }
};
template <>
struct CovAction<SpecSsi> {
    static constexpr bool BY_SLOT = false;
    MC_HD static int nbins(const SsiParams &) { return 7 + 1; }
    MC_HD static bool listed(const SsiParams &, int a) { return a >= 0 && a < 7; }
    template <class Ref>
    MC_HD static int of(const SsiParams &p, const SpecSsi::Local &l, Ref, int slot) {
        SpecSsi::Delta d;
        int action = -1;
        SpecSsi::compute(p, l, slot, d, action);
        return action;
    }
};
// compiled PlusCal: action id = the label id the slot's process instance stands at (vm_action_of, pcal_compile.cpp); the label table of
// the image has one entry per label id, "Done" — the last one — included; the terminating disjunct (the last slot) comes after them
MC_HD int cov_vm_nlabels(const VmParams &p) { return p.self_tab - p.label_tab; }
template <int MAXV>
struct CovAction<SpecVmT<MAXV>> {
    using S = SpecVmT<MAXV>;
    static constexpr bool BY_SLOT = false;
    MC_HD static int nbins(const VmParams &p) { return cov_vm_nlabels(p) + 1 + 1; }
    MC_HD static bool listed(const VmParams &p, int a) { return a >= 0 && a <= cov_vm_nlabels(p) && a != p.done; }
    template <class Ref>
    MC_HD static int of(const VmParams &p, const typename S::Local &l, Ref, int slot) {
        if (slot >= p.ninst * p.maxch) return cov_vm_nlabels(p);
        return slot < 0 ? -1 : l.v[p.pc_base + slot / p.maxch];
    }
};
template <int MAXV>
struct CovAction<SpecVmCfgT<MAXV>> : CovAction<SpecVmT<MAXV>> {};   // (spec_vm_cfg.h: the same rows and slots)
// ... as generated code: the pc cell from the stored (possibly packed) row
template <class G>
struct CovAction<SpecGenT<G>> {
    using S = SpecGenT<G>;
    static constexpr bool BY_SLOT = false;
    MC_HD static int nbins(const VmParams &) { return G::NLABELS + 1 + 1; }
    MC_HD static bool listed(const VmParams &, int a) { return a >= 0 && a <= G::NLABELS && a != G::DONE; }
    template <class Ref>
    MC_HD static int of(const VmParams &, const typename S::Local &, Ref s, int slot) {
        if (slot >= G::NINST * G::MAXCH) return G::NLABELS;
        return slot < 0 ? -1 : (int)G::pc_from_row(s, slot / G::MAXCH);
    }
};

// One expanded state on the host: add(action id) once per pair that counts.  (The device kernel is this loop with the wavefront's
// largest nslots as its bound: engine_coverage.h k_coverage_generated.)
template <class S, class Add>
inline void cov_state(const typename S::Params &prm, CWordRef s, Add &&add) {
    typename S::Local loc;
    S::load(prm, s, loc);
    const int ns = S::nslots(prm, loc);
    for (int slot = 0; slot < ns; ++slot) {
        uint64_t fp = 0;
        const unsigned st = S::eval(prm, loc, s, slot, fp);
        if (cov_counts(st)) add(CovAction<S>::of(prm, loc, s, slot));
    }
}

}  // namespace mc
