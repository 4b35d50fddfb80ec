// tests/_contshim/contshim.cpp — TEST-ONLY host build of what -continue collects (tla_rust_amd/csrc/violations.h: viol_pair,
// viol_ends_search, viol_pair_column, viol_deadlocked, viol_stored_bin, ViolModel<S>) over the spec lowerings, with g++ and no HIP: the
// very rules the device kernels of engine_violations.h run, driven by a plain sequential search that goes on past violated invariants
// and deadlocks and ends, like the engine, at the end of the level that holds a fatal pair.
//
// tests/test_continue_host.py compares the per-entry counts with the reference's state graph.  Linked against tests/_shim's libshim.so
// (the host helpers of compiled programs), like tests/_covshim.
#include "spec_registry.h"   // -I <a csrc directory>: the product's, or a copy with one edit (the mutants of tests/test_continue_host.py)
#include "violations.h"
#include <stdio.h>
#include <string.h>
#include <string>
#include <unordered_set>
#include <vector>

using namespace mc;

struct ContOut {
    uint64_t states[VIOL_BINS], outside[VIOL_BINS];
    uint64_t first_state[VIOL_BINS];      // index of the first stored violator in the order found (the dump's line), ~0 = none
    uint32_t first_level[VIOL_BINS];      // its level; for a bin with outside successors only (and the fatal bin): the level of the parent
    uint64_t first_parent[VIOL_BINS];     // outside / fatal: the smallest (parent, slot)
    uint32_t first_slot[VIOL_BINS];
    uint64_t distinct, generated;
    uint32_t depth, ninv, fatal, fatal_kind;
    uint64_t levels[4096];
};

template <class S, class = void>
struct StepStatus { static constexpr bool value = false; };
template <class S>
struct StepStatus<S, decltype((void)S::STEP_STATUS)> { static constexpr bool value = true; };

template <class S>
static int search(const typename S::Params &prm, int check_deadlock, const char *dump_path, ContOut *o) {
    const int W = S::words(prm);
    memset(o, 0, sizeof *o);
    for (int b = 0; b < VIOL_BINS; b++) o->first_state[b] = o->first_parent[b] = ~0ull;
    o->ninv = (uint32_t)ViolModel<S>::ninv(prm);
    FILE *dump = dump_path ? fopen(dump_path, "w") : nullptr;
    std::vector<char> txt(1 << 16);
    std::unordered_set<uint64_t> seen;
    std::vector<uint64_t> rows;              // every stored state, in the order found
    std::vector<int64_t> parent;
    std::vector<int> pslot;
    std::vector<uint32_t> level_of;
    auto store = [&](const uint64_t *w, unsigned level, int64_t par, int slot) {
        rows.insert(rows.end(), w, w + W);
        parent.push_back(par);
        pslot.push_back(slot);
        level_of.push_back(level);
        if (dump) {
            const int m = S::format(prm, w, txt.data(), txt.size());
            for (int i = 0; i < m; i++) if (txt[i] == '\n') txt[i] = ' ';
            fprintf(dump, "L%u %.*s\n", level, m, txt.data());
        }
    };
    // the stored pass over states [lo, hi)
    auto stored_pass = [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            const CWordRef self{&rows[i * W], 1};
            const int bin = viol_stored_bin<S>(prm, self, parent[i] >= 0,
                [&]() -> unsigned {
                    if constexpr (ViolChecksStored<S>::value) {
                        typename S::Local loc;
                        S::load(prm, self, loc);
                        if constexpr (StepStatus<S>::value) return S::parent_status_step(prm, loc, self);
                        else return S::parent_status(prm, loc, self);
                    } else return 0u;
                },
                [&]() -> unsigned {
                    const CWordRef ps{&rows[(size_t)parent[i] * W], 1};
                    typename S::Local loc;
                    S::load(prm, ps, loc);
                    uint64_t f = 0;
                    return S::eval(prm, loc, ps, pslot[i], f);
                });
            if (bin < 0) continue;
            o->states[bin]++;
            if (o->first_state[bin] == ~0ull) { o->first_state[bin] = i; o->first_level[bin] = level_of[i]; }
        }
    };
    uint64_t tmp[S::MAX_WORDS];
    for (uint64_t k = 0; k < S::num_init(prm); k++) {
        S::init(prm, k, WordRef{tmp, 1});
        o->generated++;
        const unsigned st = S::init_status(prm, CWordRef{tmp, 1});
        if (st & ST_OUT_OF_MODEL) continue;
        if (seen.insert(S::fp_of(prm, CWordRef{tmp, 1})).second) store(tmp, 1, -1, 0);
    }
    size_t lo = 0, hi = parent.size();
    o->levels[0] = hi;
    if (!ViolChecksStored<S>::value) stored_pass(0, hi);
    unsigned level = 1;
    int rc = 0;
    while (hi > lo && !rc && !o->fatal) {
        for (size_t i = lo; i < hi && !rc; i++) {
            // (a copy: `rows` grows while the state is expanded)
            std::vector<uint64_t> cur(rows.begin() + (long)(i * W), rows.begin() + (long)((i + 1) * W));
            const CWordRef s{cur.data(), 1};
            typename S::Local loc;
            S::load(prm, s, loc);
            const int ns = S::nslots(prm, loc);
            unsigned gen = 0;
            for (int slot = 0; slot < ns; slot++) {
                uint64_t fp = 0;
                const unsigned st = S::eval(prm, loc, s, slot, fp);
                if (!(st & ST_ENABLED)) continue;
                gen++;
                o->generated++;
                if (st & ST_OVERFLOW) { rc = MC_EOVERFLOW; break; }
                const ViolPair r = viol_pair<S>(st);
                const int column = viol_pair_column(r);
                auto note_pair = [&](int bin) {
                    if (o->first_parent[bin] == ~0ull) { o->first_parent[bin] = i; o->first_slot[bin] = (uint32_t)slot; if (!o->states[bin]) o->first_level[bin] = level; }
                };
                if (column == 1) { o->outside[r.bin]++; note_pair((int)r.bin); }
                else if (column == 0) { o->states[r.bin]++; if (o->first_state[r.bin] == ~0ull) { o->first_state[r.bin] = i; o->first_level[r.bin] = level; } }
                if (viol_ends_search(r)) {
                    if (!o->fatal) { o->fatal = 1; o->fatal_kind = r.kind; }
                    o->outside[VIOL_BIN_FATAL]++;
                    note_pair(VIOL_BIN_FATAL);
                }
                if (st & (ST_ASSERT | ST_SPECERR | ST_OUT_OF_MODEL | ST_SELFLOOP)) continue;
                if (seen.insert(fp).second) {
                    S::apply(prm, s, slot, WordRef{tmp, 1});
                    store(tmp, level + 1, (int64_t)i, slot);
                }
            }
            if (viol_deadlocked(gen, check_deadlock != 0)) {
                o->states[VIOL_BIN_DEADLOCK]++;
                if (o->first_state[VIOL_BIN_DEADLOCK] == ~0ull) { o->first_state[VIOL_BIN_DEADLOCK] = i; o->first_level[VIOL_BIN_DEADLOCK] = level; }
            }
        }
        const size_t new_hi = parent.size();
        if (ViolChecksStored<S>::value) stored_pass(lo, hi);
        else stored_pass(hi, new_hi);
        lo = hi;
        hi = new_hi;
        if (hi > lo) { if (level < 4096) o->levels[level] = hi - lo; level++; }
        if (level >= 4095) rc = -4;
    }
    if (dump) fclose(dump);
    o->distinct = parent.size();
    o->depth = level;
    return rc;
}

extern "C" int contshim_search(const mc_spec_desc *d, int check_deadlock, const char *dump_path, ContOut *out) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) { return search<decltype(spec)>(prm, check_deadlock, dump_path, out); });
}
