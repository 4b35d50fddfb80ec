// tests/_sideshim/sidehost.cpp — TEST-ONLY host build (g++, no HIP) of the product's own host loops over the table lowering of
// spec_table.h: graph_state / graph_edge / seen_find (graph.h), cov_state (coverage.h), viol_stored_bin / viol_pair / viol_pair_column /
// viol_ends_search / viol_deadlocked (violations.h), live_edge_unit and the LiveProc / LivePred traits (liveness.h), on the rows the
// device tests use.  It fills the very arrays tests/_sideshim/sideshim.hip returns, so that tests/test_sidepass_reference.py holds
// tests/sidemodel.py against the shared MC_HD rules on this machine, and tests/test_gpu_sidepasses.py holds the kernels against the
// model.  What only device headers define is restated here, each with its origin: graph_bad_key and GRAPH_NO_INDEX (engine_graph.h),
// viol_key (engine_kernels.h), the cells of ViolBins (engine_violations.h).
#include "spec_registry.h"
#include "graph.h"
#include "liveness.h"
#include "violations.h"
#include "spec_table.h"
#include <string.h>
#include <vector>

using namespace mc;

namespace {
constexpr uint32_t NO_INDEX = 0xffffffffu;                                                        // engine_graph.h: GRAPH_NO_INDEX
uint64_t bad_key(uint64_t idx, unsigned slot) { return (idx << 16) | (slot & 0xffffu); }         // engine_graph.h: graph_bad_key
uint64_t vkey(uint64_t idx, unsigned slot, unsigned kind, unsigned inv) {                         // engine_kernels.h: viol_key
    return ((slot & 0xffffu) == 0xfffdu ? 0ull : 1ull << 62) | (idx << 24) | ((uint64_t)(slot & 0xffffu) << 8) | ((inv & 31u) << 3) | kind;
}
struct Gc { uint64_t missing_states = 0, missing_succ = 0, first_bad = ~0ull, dropped = 0, self_loops = 0, max_degree = 0; };
void gc_out(const Gc &g, uint64_t *o) { o[0] = g.missing_states; o[1] = g.missing_succ; o[2] = g.first_bad; o[3] = g.dropped; o[4] = g.self_loops; o[5] = g.max_degree; }
void note(uint64_t *bins, int cell, uint64_t key) {   // engine_violations.h: ViolBins = count[2 * VIOL_BINS], then first[2 * VIOL_BINS]
    if (cell < 0 || cell >= 2 * VIOL_BINS) return;
    bins[cell]++;
    if (key < bins[2 * VIOL_BINS + cell]) bins[2 * VIOL_BINS + cell] = key;
}

template <class S>
void violations(const SpecTabParams &prm, const uint64_t *rows, const uint32_t *parent, const uint16_t *pslot, uint64_t lo, uint64_t hi, uint64_t new_hi,
                int expanded, unsigned flags, uint64_t *bins) {
    const int W = S::words(prm);
    auto stored = [&](uint64_t a, uint64_t b) {
        for (uint64_t i = a; i < b; i++) {
            const CWordRef self{rows + i * W, 1};
            uint32_t p = 0xffffffffu;
            if (!ViolChecksStored<S>::value) p = parent[i];
            const bool has_parent = p != 0xffffffffu;
            if (has_parent && p >= i) continue;   // a record that cannot be one is counted nowhere
            const int bin = viol_stored_bin<S>(prm, self, has_parent,
                [&]() -> unsigned {
                    typename S::Local loc;
                    S::load(prm, self, loc);
                    return S::parent_status(prm, loc, self);
                },
                [&]() -> unsigned {
                    const CWordRef ps{rows + (uint64_t)p * W, 1};
                    typename S::Local loc;
                    S::load(prm, ps, loc);
                    uint64_t f = 0;
                    return S::eval(prm, loc, ps, (int)pslot[i], f);
                });
            if (bin >= 0) note(bins, bin, i);
        }
    };
    if (expanded)
        for (uint64_t i = lo; i < hi; i++) {
            const CWordRef s{rows + i * W, 1};
            typename S::Local loc;
            S::load(prm, s, loc);
            const int ns = S::nslots(prm, loc);
            unsigned gen = 0;
            for (int slot = 0; slot < ns; slot++) {
                uint64_t f = 0;
                const unsigned st = S::eval(prm, loc, s, slot, f);
                if (st & ST_ENABLED) gen++;
                const ViolPair r = viol_pair<S>(st);
                const uint64_t key = vkey(i, (unsigned)slot, r.kind, r.inv);
                const int column = viol_pair_column(r);
                if (column >= 0) note(bins, column * VIOL_BINS + (int)r.bin, key);
                if (viol_ends_search(r)) note(bins, VIOL_BINS + VIOL_BIN_FATAL, key);
            }
            if (viol_deadlocked(gen, (flags & MC_F_DEADLOCK) != 0)) note(bins, VIOL_BIN_DEADLOCK, i);
        }
    if (!expanded || ViolChecksStored<S>::value) stored(lo, hi);
    else stored(hi, new_hi);
}
}  // namespace

extern "C" {

// the arguments and outputs of sd_graph (sideshim.hip); table: 16-byte aligned
int sh_graph(const SpecTabParams *prm_, const uint64_t *rows, uint64_t n, uint64_t expanded, const uint64_t *table, uint64_t nbuckets, int sparse,
             const int8_t *unit_tab, int nlabels, int npred, uint64_t cap, uint32_t *slot_index, uint32_t *degree, uint64_t *offsets, uint32_t *dst,
             int16_t *act, int8_t *proc, int8_t *unit, uint32_t *pred, uint64_t *gc_degree, uint64_t *gc_fill, uint64_t *pred_bad, uint64_t *edges_out) {
    using S = SpecTab;
    const SpecTabParams prm = *prm_;
    const int W = S::words(prm);
    const uint64_t table_cap = nbuckets * (uint64_t)(sparse ? MC_SPARSE_SLOTS : 8), seen = sparse ? (nbuckets | GRAPH_SEEN_SPARSE) : nbuckets;
    Gc gc;
    for (uint64_t k = 0; k < table_cap; k++) slot_index[k] = NO_INDEX;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t pos = seen_find(table, seen, S::fp_of(prm, CWordRef{rows + i * W, 1}));
        if (pos < table_cap) slot_index[pos] = (uint32_t)i;
        else { gc.missing_states++; if (bad_key(i, 0xffffu) < gc.first_bad) gc.first_bad = bad_key(i, 0xffffu); }
    }
    for (uint64_t i = 0; i <= n; i++) degree[i] = 0;
    for (uint64_t i = 0; i < expanded; i++) {
        uint32_t deg = 0;
        graph_state<S>(prm, CWordRef{rows + i * W, 1}, table, seen, [&](unsigned kind, uint64_t, int, int slot) {
            if (kind == GE_SELF || kind == GE_EDGE) deg++;
            else if (kind == GE_DROPPED) gc.dropped++;
            else if (kind == GE_MISSING) { gc.missing_succ++; if (bad_key(i, (unsigned)slot) < gc.first_bad) gc.first_bad = bad_key(i, (unsigned)slot); }
        });
        degree[i] = deg;
        if (deg > gc.max_degree) gc.max_degree = deg;
    }
    uint64_t run = 0;
    for (uint64_t i = 0; i <= n; i++) { offsets[i] = run; run += degree[i]; }
    *edges_out = run;
    gc_out(gc, gc_degree);
    if (run > cap) return -1;
    LiveUnitTab utab{prm.ninst, nlabels, unit_tab};
    for (uint64_t i = 0; i < expanded; i++) {
        const CWordRef s{rows + i * W, 1};
        S::Local loc;
        S::load(prm, s, loc);
        uint64_t out = offsets[i];
        graph_state<S>(prm, s, table, seen, [&](unsigned kind, uint64_t pos, int action, int slot) {
            if (kind == GE_MISSING) { gc.missing_succ++; if (bad_key(i, (unsigned)slot) < gc.first_bad) gc.first_bad = bad_key(i, (unsigned)slot); }
            if (kind != GE_SELF && kind != GE_EDGE) return;
            uint32_t to = (uint32_t)i;
            if (kind == GE_EDGE) {
                to = pos < table_cap ? slot_index[pos] : NO_INDEX;
                if (to == NO_INDEX) { gc.missing_succ++; if (bad_key(i, (unsigned)slot) < gc.first_bad) gc.first_bad = bad_key(i, (unsigned)slot); }
            }
            if (to == (uint32_t)i) gc.self_loops++;
            dst[out] = to;
            act[out] = (int16_t)action;
            proc[out] = (int8_t)LiveProc<S>::of(prm, slot);
            unit[out] = (int8_t)live_edge_unit<S>(prm, loc, utab, slot);
            out++;
        });
    }
    gc_out(gc, gc_fill);
    uint64_t pbad = ~0ull;
    LivePredTab ptab;
    memset(&ptab, 0, sizeof ptab);
    ptab.n = npred;
    for (uint64_t i = 0; i < n; i++) {
        S::Local loc;
        S::load(prm, CWordRef{rows + i * W, 1}, loc);
        uint32_t bits = 0;
        for (int k = 0; k < npred; k++) {
            int32_t res = 0;
            if (!LivePred<S>::eval(prm, loc, ptab, k, res)) { if ((i << 8 | (unsigned)k) < pbad) pbad = i << 8 | (unsigned)k; continue; }
            if (res) bits |= 1u << k;
        }
        pred[i] = npred ? bits : 0;
    }
    *pred_bad = pbad;
    return 0;
}

// the arguments and outputs of sd_coverage
int sh_coverage(const SpecTabParams *prm_, const uint64_t *rows, uint64_t n, const uint32_t *parent, const uint16_t *pslot, uint64_t gen_lo, uint64_t gen_hi,
                uint64_t dist_lo, uint64_t dist_hi, uint64_t *bins) {
    using S = SpecTab;
    const SpecTabParams prm = *prm_;
    const int W = S::words(prm), nbins = CovAction<S>::nbins(prm);
    (void)n;
    auto bump = [&](uint64_t *b, int bin) { if (bin >= 0 && bin < nbins) b[bin]++; };
    for (uint64_t i = gen_lo; i < gen_hi; i++) cov_state<S>(prm, CWordRef{rows + i * W, 1}, [&](int a) { bump(bins, a + 1); });
    for (uint64_t i = dist_lo; i < dist_hi; i++) {
        const uint32_t p = parent[i];
        if (p == 0xffffffffu) { bump(bins + nbins, 0); continue; }
        if (p >= i) continue;   // a record that cannot be one
        const CWordRef s{rows + (uint64_t)p * W, 1};
        S::Local loc;
        S::load(prm, s, loc);
        bump(bins + nbins, CovAction<S>::of(prm, loc, s, (int)pslot[i]) + 1);
    }
    return 0;
}

// the arguments and outputs of sd_violations
int sh_violations(int stored_variant, const SpecTabParams *prm, const uint64_t *rows, uint64_t n, const uint32_t *parent, const uint16_t *pslot, uint64_t lo,
                  uint64_t hi, uint64_t new_hi, int expanded, unsigned flags, uint64_t *bins) {
    (void)n;
    if (stored_variant) violations<SpecTabStored>(*prm, rows, parent, pslot, lo, hi, new_hi, expanded, flags, bins);
    else violations<SpecTab>(*prm, rows, parent, pslot, lo, hi, new_hi, expanded, flags, bins);
    return 0;
}

}  // extern "C"
