// tests/_strongshim/strongshim.cpp — TEST-ONLY host build of the rule by which liveness under strong fairness of whole processes is
// decided (tla_rust_amd/csrc/liveness.h: live_enabled_in, live_blockers, live_classify, live_violates_strong, live_refine_state /
// live_closes_state, live_strong_rounds, beside the functions of the weak rule) over the compiled-program lowering, with g++ and no HIP:
// the very functions the kernels of engine_live.h call.  As tests/_livepropshim does, a plain sequential search fills a table in the
// seen-set's layout, graph.h gives every state's row and LiveProc the process of every edge.  What the device does in parallel is
// sequential here: every round's components come from a Tarjan over the edges between open states.
//
// tests/test_strongfair_host.py compares the verdict, the final components, the refined ids, the rounds, the closed states and the
// witness with tests/strongfair.py by state TEXT, and builds this file against copies of csrc with one edit each (the mutants).
// Linked against tests/_shim's libshim.so.
#include "spec_registry.h"   // -I <a csrc directory>: the product's, or a copy with one edit
#include "liveness.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace mc;

static uint64_t host_insert(uint64_t *table, uint64_t nbuckets, uint64_t fp, bool *fresh) {   // (tests/_graphshim: the 8-slot form)
    uint64_t bk = ((fp & 0xffffffffull) * nbuckets) >> 32;
    const unsigned j0 = (unsigned)(fp >> 32) & 7u;
    for (uint64_t probe = 0; probe < 2048 && probe < nbuckets; ++probe) {
        for (int i = 0; i < 8; i++)
            if (table[bk * 8 + i] == fp) { *fresh = false; return bk * 8 + i; }
        for (unsigned r = 0; r < 8; r++) {
            const unsigned i = (j0 + r) & 7u;
            if (table[bk * 8 + i] == 0) { table[bk * 8 + i] = fp; *fresh = true; return bk * 8 + i; }
        }
        bk = bk + 1 == nbuckets ? 0 : bk + 1;
    }
    return ~0ull;
}

// comp[v] = the least vertex of v's component, over the edges u -> w with keep[u] and keep[w] (iterative Tarjan over CSR rows)
static void tarjan(const std::vector<uint64_t> &off, const std::vector<uint32_t> &dst, const std::vector<char> &keep, std::vector<uint32_t> &comp) {
    const size_t n = off.size() - 1;
    std::vector<int64_t> index(n, -1), low(n, 0);
    std::vector<char> on(n, 0);
    std::vector<uint32_t> stack;
    std::vector<std::pair<uint32_t, uint64_t>> work;
    comp.assign(n, 0);
    int64_t count = 0;
    for (size_t root = 0; root < n; root++) {
        if (index[root] >= 0) continue;
        index[root] = low[root] = count++;
        stack.push_back((uint32_t)root);
        on[root] = 1;
        work.push_back({(uint32_t)root, off[root]});
        while (!work.empty()) {
            const uint32_t v = work.back().first;
            bool advanced = false;
            while (work.back().second < off[v + 1]) {
                const uint32_t w = dst[work.back().second++];
                if (!keep[v] || !keep[w]) continue;
                if (index[w] < 0) {
                    index[w] = low[w] = count++;
                    stack.push_back(w);
                    on[w] = 1;
                    work.push_back({w, off[w]});
                    advanced = true;
                    break;
                }
                if (on[w] && index[w] < low[v]) low[v] = index[w];
            }
            if (advanced) continue;
            work.pop_back();
            if (!work.empty() && low[v] < low[work.back().first]) low[work.back().first] = low[v];
            if (low[v] == index[v]) {
                size_t first = stack.size();
                uint32_t least = v;
                do { --first; on[stack[first]] = 0; if (stack[first] < least) least = stack[first]; } while (stack[first] != v);
                for (size_t k = first; k < stack.size(); k++) comp[stack[k]] = least;
                stack.resize(first);
            }
        }
    }
}

// kind < 0: Termination.  states_path: one line per state, its text; out_path: one line per state "<refined id> <0 closed, 2 final>
// <dist, -1 = none>".  counts: [0] states, [1] final violating components, [2] the witness (~0 = none; Termination: the least final
// root), [3] rounds, [4] states in M, [5] bad starts, [6] states closed, [7] 1 = the refinement ran into its bound
template <class S>
static int check(const typename S::Params &prm, uint64_t weak, uint64_t strong, int kind, int p, int q, const char *states_path, const char *out_path, uint64_t *counts) {
    if constexpr (!LiveProc<S>::HAS || !LivePred<S>::HAS) {
        return MC_ENOSPEC;
    } else {
        const int W = S::words(prm);
        const uint64_t nbuckets = 1 << 13, seen = nbuckets;
        uint64_t *table = (uint64_t *)aligned_alloc(64, (size_t)nbuckets * 8 * sizeof(uint64_t));
        if (!table) return -4;
        memset(table, 0, (size_t)nbuckets * 8 * sizeof(uint64_t));
        std::vector<uint32_t> slot_index((size_t)nbuckets * 8, 0xffffffffu);
        std::vector<uint64_t> rows;
        size_t n = 0, ninit = 0;
        int rc = 0;
        auto put = [&](uint64_t fp, const uint64_t *w) {
            bool fresh = false;
            const uint64_t pos = host_insert(table, nbuckets, fp, &fresh);
            if (pos == ~0ull) { rc = MC_ETABLEFULL; return; }
            if (!fresh) return;
            slot_index[pos] = (uint32_t)n++;
            rows.insert(rows.end(), w, w + W);
        };
        uint64_t tmp[S::MAX_WORDS];
        for (uint64_t k = 0; k < S::num_init(prm) && !rc; k++) {
            S::init(prm, k, WordRef{tmp, 1});
            if (S::init_status(prm, CWordRef{tmp, 1}) & ST_OUT_OF_MODEL) continue;
            put(S::fp_of(prm, CWordRef{tmp, 1}), tmp);
        }
        ninit = n;
        for (size_t i = 0; i < n && !rc; i++) {
            std::vector<uint64_t> cur(rows.begin() + i * W, rows.begin() + (i + 1) * W);
            const CWordRef s{cur.data(), 1};
            typename S::Local loc;
            S::load(prm, s, loc);
            const int ns = S::nslots(prm, loc);
            for (int slot = 0; slot < ns && !rc; slot++) {
                uint64_t fp = 0;
                const unsigned st = S::eval(prm, loc, s, slot, fp);
                if (!(st & ST_ENABLED) || (st & (ST_ASSERT | ST_SPECERR | ST_OVERFLOW | ST_OUT_OF_MODEL | ST_SELFLOOP))) continue;
                S::apply(prm, s, slot, WordRef{tmp, 1});
                put(fp, tmp);
            }
        }
        // rows of the graph with the process of every edge, and the predicate bits of every state
        std::vector<uint64_t> off(n + 1, 0);
        std::vector<uint32_t> dst, bits(n, 0);
        std::vector<char> done(n, 0);
        std::vector<int8_t> proc;
        LivePredTab tab;
        memset(&tab, 0, sizeof tab);
        tab.n = vm_live_preds(prm.host, tab.entry, LIVE_MAX_PREDS);
        if (tab.n > LIVE_MAX_PREDS) rc = MC_EBADCFG;
        for (size_t i = 0; i < n && !rc; i++) {
            graph_state<S>(prm, CWordRef{&rows[i * W], 1}, table, seen, [&](unsigned kd, uint64_t pos, int, int slot) {
                if (kd != GE_SELF && kd != GE_EDGE) return;
                const uint32_t to = kd == GE_SELF ? (uint32_t)i : slot_index[pos];
                if (to == 0xffffffffu) { rc = MC_ESTATE; return; }
                dst.push_back(to);
                proc.push_back((int8_t)LiveProc<S>::of(prm, slot));
                if (proc.back() == LIVE_TERM) done[i] = 1;
            });
            off[i + 1] = dst.size();
            typename S::Local loc;
            S::load(prm, CWordRef{&rows[i * W], 1}, loc);
            for (int k = 0; k < tab.n; k++) {
                int32_t res = 0;
                if (!LivePred<S>::eval(prm, loc, tab, k, res)) { rc = MC_ESTATE; break; }
                if (res) bits[i] |= 1u << k;
            }
        }
        if (rc) { free(table); return rc; }
        const bool term = kind < 0;
        const LiveCheck ck{term ? LIVE_STABLE : kind, p, q};
        const int np = LiveProc<S>::count(prm);
        const uint64_t all = np >= 64 ? ~0ull : (1ull << np) - 1;
        auto in_m = [&](uint32_t d) { return term || live_in_mask(ck, bits[d]); };
        auto target = [&](uint32_t d) { return term ? !done[d] : live_in_target(ck, bits[d]); };
        memset(counts, 0, 8 * sizeof(uint64_t));
        // ---- the refinement: every state of M open; per round the components of the open subgraph, the rule per component
        std::vector<uint8_t> open(n);
        std::vector<uint32_t> ids(n), dist(n, LIVE_FAR), comp;
        for (size_t i = 0; i < n; i++) { open[i] = in_m((uint32_t)i) ? LIVE_ST_OPEN : LIVE_ST_CLOSED; ids[i] = (uint32_t)i; if (open[i]) counts[4]++; }
        const uint32_t bound = live_strong_rounds(all, strong);
        uint64_t first_root = ~0ull;
        for (uint32_t round = 1;; round++) {
            counts[3] = round;
            std::vector<char> keep(n);
            for (size_t i = 0; i < n; i++) keep[i] = open[i] == LIVE_ST_OPEN;
            tarjan(off, dst, keep, comp);
            std::vector<LiveComp> entry(n);
            std::vector<uint64_t> enabled(n, 0), en_of(n, 0);
            for (size_t i = 0; i < n; i++) {
                if (!keep[i]) continue;
                uint64_t en = 0, taken = 0;
                live_state_masked((uint32_t)i, dst.data() + off[i], proc.data() + off[i], off[i + 1] - off[i], comp.data(), [&](uint32_t d) { return keep[d] != 0; }, &en, &taken);
                en_of[i] = live_enabled_in((uint32_t)i, dst.data() + off[i], proc.data() + off[i], off[i + 1] - off[i], comp.data());
                live_merge(entry[comp[i]], taken, live_disabled(all, en), target((uint32_t)i));
                enabled[comp[i]] |= en_of[i];
            }
            bool still = false;
            for (size_t i = 0; i < n; i++) {
                if (!keep[i]) continue;
                const LiveComp &c = entry[comp[i]];
                const int cls = live_classify(all, weak, strong, c.taken, c.disabled, enabled[comp[i]], c.done, c.size);
                if (comp[i] == i && live_violates_strong(all, weak, strong, c.taken, c.disabled, enabled[comp[i]], c.done, c.size)) {
                    counts[1]++;
                    if (i < first_root) first_root = i;
                }
                open[i] = live_refine_state(cls, live_blockers(all, strong, enabled[comp[i]], c.taken), en_of[i]);
                if (open[i] == LIVE_ST_FINAL) { ids[i] = comp[i]; dist[i] = 0; }
                if (open[i] == LIVE_ST_CLOSED) counts[6]++;
                if (open[i] == LIVE_ST_OPEN) still = true;
            }
            if (!still) break;
            if (round >= bound) { counts[7] = 1; break; }
        }
        counts[0] = n;
        counts[2] = term ? first_root : ~0ull;
        if (!term) {
            // ---- reach, to a fixed point, and the witness
            auto passable = [&](uint32_t d) { return live_passable(ck, bits[d]); };
            for (bool changed = true; changed;) {
                changed = false;
                for (size_t i = 0; i < n; i++) {
                    if (!passable((uint32_t)i) || dist[i] == 0) continue;
                    const uint32_t best = live_reach_step((uint32_t)i, dist[i], dst.data() + off[i], off[i + 1] - off[i], dist.data(), passable);
                    if (best < dist[i]) { dist[i] = best; changed = true; }
                }
            }
            for (size_t i = n; i-- > 0;)
                if (in_m((uint32_t)i) && dist[i] != LIVE_FAR && live_in_start(ck, bits[i], i < ninit)) { counts[2] = i; counts[5]++; }
        }
        FILE *fs = fopen(states_path, "w"), *fo = fopen(out_path, "w");
        if (!fs || !fo) rc = -5;
        std::vector<char> txt(1 << 16);
        for (size_t i = 0; i < n && !rc; i++) {
            const int m = S::format(prm, &rows[i * W], txt.data(), txt.size());
            for (int k = 0; k < m; k++) if (txt[k] == '\n') txt[k] = ' ';
            fprintf(fs, "%.*s\n", m, txt.data());
            fprintf(fo, "%u %d %lld\n", ids[i], (int)open[i], dist[i] == LIVE_FAR ? -1ll : (long long)dist[i]);
        }
        if (fs) fclose(fs);
        if (fo) fclose(fo);
        free(table);
        return rc;
    }
}

extern "C" int strongshim_check(const mc_spec_desc *d, uint64_t weak, uint64_t strong, int kind, int p, int q, const char *states_path, const char *out_path,
                                uint64_t *counts) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) { return check<decltype(spec)>(prm, weak, strong, kind, p, q, states_path, out_path, counts); });
}
