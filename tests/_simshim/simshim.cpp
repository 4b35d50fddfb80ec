// tests/_simshim/simshim.cpp — TEST-ONLY host build of simulation mode's walk (tla_rust_amd/csrc/sim_walk.h) over the spec
// lowerings, with g++ and no HIP: the very sim_step the device kernel k_simulate runs, driven one walk at a time.
//
// tests/test_simulate_host.py checks these walks against the CPU oracle (every state a walk reaches is one the BFS stores);
// tests/test_gpu_simulate.py checks that the device's walks are these walks.  The PlusCal front-end (vm_make_params and the other
// host helpers of a compiled program) is not compiled in: the library is linked against tests/_shim's libshim.so, so that its program
// handles (helpers.ShimProgram) can be walked here.
#include "spec_registry.h"   // -I <a csrc directory>: the product's, or a copy with an edited sim_walk.h (the mutants of
#include "sim_walk.h"        // tests/test_simulate_graph.py)
#include <stdio.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>

using namespace mc;

struct SimShimOut {
    uint64_t generated, steps, walks, viol;   // counters of the walks run; viol: the least violation key, ~0 = none
    uint32_t max_depth, pad;
};

// walks first .. first+n-1: slots[k * depth + s] (slot from state s to s + 1, -1 beyond the walk), len[k], end[k]; dump_path: one
// line "S<t> <state text>" per state reached (t = 1 for the initial state); rows_walk: the states of that walk as plain rows into
// rows (depth * words), plus the successor that breaks an invariant; that successor of any walk is also a dump line "V<t> <text>"
// after the walk's last state; dump_ids: a text is written once, as "#<id> <text>" where it first occurs and "#<id>" after that (a million
// walks of a small model are a few thousand texts); gen[k], viol[k]: the walk's own `generated` and violation key (~0 = none)
template <class S>
static int walks(const typename S::Params &prm, uint64_t seed, uint64_t first, uint64_t n, uint32_t depth, int deadlock, const char *dump_path, int dump_ids,
                 int32_t *slots, uint32_t *len, uint32_t *end, uint64_t rows_walk, uint64_t *rows, SimShimOut *o, uint32_t *gen, uint64_t *viol) {
    const int W = S::words(prm);
    std::vector<uint64_t> buf[2] = {std::vector<uint64_t>(W), std::vector<uint64_t>(W)};
    FILE *dump = dump_path ? fopen(dump_path, "w") : nullptr;
    std::vector<char> txt(1 << 16);
    std::unordered_map<std::string, unsigned> ids;   // keyed by the row's words: a row is formatted where it first occurs only
    auto put = [&](char tag, unsigned t, const uint64_t *row) {
        if (dump_ids) {
            const auto it = ids.emplace(std::string((const char *)row, (size_t)W * sizeof(uint64_t)), (unsigned)ids.size());
            if (!it.second) { fprintf(dump, "%c%u #%u\n", tag, t, it.first->second); return; }
            fprintf(dump, "%c%u #%u ", tag, t, it.first->second);
        } else fprintf(dump, "%c%u ", tag, t);
        const int m = S::format(prm, row, txt.data(), txt.size());
        for (int i = 0; i < m; i++) if (txt[i] == '\n') txt[i] = ' ';
        fprintf(dump, "%.*s\n", m, txt.data());
    };
    memset(o, 0, sizeof *o);
    o->viol = ~0ull;
    for (uint64_t k = 0; k < n; ++k) {
        SimWalk wk;
        sim_begin(wk, seed, first + k, 0, SIM_RUNNING);
        if (slots) for (uint32_t s = 0; s < depth; ++s) slots[k * depth + s] = -1;
        const bool keep = rows && first + k == rows_walk;
        while (wk.end == SIM_RUNNING) {
            const uint32_t t = wk.t;
            const CWordRef cur{buf[(t + 1) & 1].data(), 1};
            const WordRef nxt{buf[t & 1].data(), 1};
            sim_step<S>(prm, wk, depth, (unsigned)deadlock, cur, nxt, [](int ns) { return ns; });
            if (wk.t > t) {
                o->steps++;
                if (dump) put('S', wk.t, nxt.p);
                if (keep) memcpy(rows + (size_t)(wk.t - 1) * W, nxt.p, W * sizeof(uint64_t));
            }
            if (slots && wk.slot >= 0) slots[k * depth + wk.t - 2] = wk.slot;
            if (wk.end == SIM_END_VIOLATION && sim_key_kind(wk.viol) == SIM_VK_INVARIANT && sim_key_slot(wk.viol) < SIM_SLOT_PARENT) {
                if (keep) S::apply(prm, cur, (int)sim_key_slot(wk.viol), WordRef{rows + (size_t)t * W, 1});
                if (dump) {
                    S::apply(prm, cur, (int)sim_key_slot(wk.viol), nxt);
                    put('V', t + 1, nxt.p);
                }
            }
        }
        o->generated += wk.gen;
        o->walks++;
        if (wk.t > o->max_depth) o->max_depth = wk.t;
        if (wk.viol < o->viol) o->viol = wk.viol;
        if (len) len[k] = wk.t;
        if (end) end[k] = wk.end;
        if (gen) gen[k] = wk.gen;
        if (viol) viol[k] = wk.viol;
    }
    if (dump) fclose(dump);
    return 0;
}

extern "C" int simshim_walks(const mc_spec_desc *d, uint64_t seed, uint64_t first, uint64_t n, uint32_t depth, int deadlock, const char *dump_path, int dump_ids,
                             int32_t *slots, uint32_t *len, uint32_t *end, uint64_t rows_walk, uint64_t *rows, SimShimOut *o, uint32_t *gen, uint64_t *viol) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) {
        return walks<decltype(spec)>(prm, seed, first, n, depth, deadlock, dump_path, dump_ids, slots, len, end, rows_walk, rows, o, gen, viol);
    });
}
extern "C" int simshim_format(const mc_spec_desc *d, const uint64_t *row, char *buf, size_t cap) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) { return decltype(spec)::format(prm, row, buf, cap); });
}
extern "C" int simshim_words(const mc_spec_desc *d) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) { return decltype(spec)::words(prm); });
}
