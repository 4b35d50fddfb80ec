// tests/_unitshim/unitshim.cpp — TEST-ONLY host build of the checks label by label with g++ and no HIP: the front end's
// unit map and conjuncts (pcal.cpp / pcal_compile.cpp, compiled in: a copy with one edit is a mutant), the unit of every edge as
// k_live_unit<S> computes it (liveness.h: live_edge_unit over LiveProc / LiveLabel / live_unit_of on the interpreter lowering's own
// load), and the rule over units (live_state_masked_units, live_enabled_in_units, beside the functions of the strong rule).  As
// tests/_strongshim does, a plain sequential search fills a table in the seen-set's layout and graph.h gives every state's row; every
// round's components come from a Tarjan over the edges between open states.
//
// tests/test_labelfair_host.py compares the verdict, the final components, the rounds, the closed states and the conjuncts of every
// edge with tests/labelfair.py by state TEXT, and builds this file against copies of csrc with one edit each (the mutants).
#include "spec_registry.h"   // -I <a csrc directory>: the product's, or a copy with one edit
#include "liveness.h"
#include "pcal.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

using namespace mc;

static std::string g_error;
extern "C" void mc_set_error_internal(const char *msg) { g_error = msg ? msg : ""; }   // (what the product's headers report through)
extern "C" const char *unitshim_error() { return g_error.c_str(); }
// the module compiled with the cfg's PROPERTY names other than Termination (comma separated); null + unitshim_error() when refused
extern "C" void *unitshim_compile(const char *tla_text, const char *properties) {
    pcal::Config cf;
    std::string cur;
    for (const char *p = properties ? properties : "";; p++) {
        if (*p == ',' || !*p) { if (!cur.empty()) cf.properties.push_back(cur); cur.clear(); if (!*p) break; }
        else cur += *p;
    }
    pcal::Module m;
    const std::string text(tla_text);
    g_error = pcal::parse_module(text, m);
    if (!g_error.empty()) return nullptr;
    auto *P = new pcal::Program();
    g_error = pcal::compile(m, text, cf, *P);
    if (!g_error.empty()) { delete P; return nullptr; }
    return P;
}
extern "C" void unitshim_free(void *p) { delete (pcal::Program *)p; }
// frontend.cpp's mc_program_fairness_units; texts: the conjuncts' texts, one per line; returns the number of conjuncts, -1 when refused
extern "C" int unitshim_table(void *prog, mc_fair_units *out, char *texts, size_t cap) {
    const pcal::Program &P = *(const pcal::Program *)prog;
    memset(out, 0, sizeof *out);
    out->nunits = (int32_t)(P.conj_of_unit.size() > 127 ? 127 : P.conj_of_unit.size());
    out->nconj = (int32_t)P.fair_conj.size();
    for (int u = 0; u < out->nunits; u++) out->of_unit[u] = P.conj_of_unit[(size_t)u];
    std::string all;
    for (size_t k = 0; k < P.fair_conj.size(); k++) { (P.fair_conj[k].strong ? out->strong_mask : out->weak_mask) |= 1ull << k; all += P.fair_conj[k].text + "\n"; }
    snprintf(texts, cap, "%s", all.c_str());
    if (!P.live_refusal_units.empty()) { g_error = P.live_refusal_units; return -1; }
    return out->nconj;
}

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

// kind < 0: Termination.  states_path: one line per state, its text; out_path: one line per state "<refined id> <0 closed, 2 final>";
// edges_path: one line per edge "<source> <successor> <unit> <the unit's conjuncts, hex>".  counts: [0] states, [1] final violating
// components, [2] the least final root (~0 = none), [3] rounds, [4] states in M, [5] 1 = violated (a final component is reached
// inside M from an S state of M; Termination: there is one), [6] states closed, [7] 1 = the refinement ran into its bound
template <class S>
static int check(const typename S::Params &prm, const mc_fair_units &fu, int kind, int p, int q, const char *states_path, const char *out_path, const char *edges_path,
                 uint64_t *counts) {
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
        // the (instance, label) -> unit table, as the engine hands it to k_live_unit<S>
        int ni = 0, nl = 0;
        vm_live_units(prm.host, &ni, &nl, nullptr, 0);
        std::vector<int8_t> unit_tab((size_t)ni * (size_t)nl + 1, (int8_t)LIVE_TERM);
        vm_live_units(prm.host, &ni, &nl, unit_tab.data(), (int)unit_tab.size());
        const LiveUnitTab utab{ni, nl, unit_tab.data()};
        // rows of the graph with the unit of every edge, and the predicate bits of every state
        std::vector<uint64_t> off(n + 1, 0);
        std::vector<uint32_t> dst, bits(n, 0);
        std::vector<char> done(n, 0);
        std::vector<int8_t> unit;
        LivePredTab tab;
        memset(&tab, 0, sizeof tab);
        tab.n = vm_live_preds(prm.host, tab.entry, LIVE_MAX_PREDS);
        if (tab.n > LIVE_MAX_PREDS) rc = MC_EBADCFG;
        for (size_t i = 0; i < n && !rc; i++) {
            typename S::Local src_row;
            S::load(prm, CWordRef{&rows[i * W], 1}, src_row);
            graph_state<S>(prm, CWordRef{&rows[i * W], 1}, table, seen, [&](unsigned kd, uint64_t pos, int, int slot) {
                if (kd != GE_SELF && kd != GE_EDGE) return;
                const uint32_t to = kd == GE_SELF ? (uint32_t)i : slot_index[pos];
                if (to == 0xffffffffu) { rc = MC_ESTATE; return; }
                typename S::Local dst_row;   // (the successor's row: no part of the rule — the mutant that reads the label there needs it)
                S::load(prm, CWordRef{&rows[(size_t)to * W], 1}, dst_row);
                (void)dst_row;
                dst.push_back(to);
                unit.push_back((int8_t)live_edge_unit<S>(prm, src_row, utab, slot));
                if (unit.back() == LIVE_TERM) done[i] = 1;
                if (unit.back() >= fu.nunits) rc = MC_EBADCFG;
            });
            off[i + 1] = dst.size();
            for (int k = 0; k < tab.n; k++) {
                int32_t res = 0;
                if (!LivePred<S>::eval(prm, src_row, tab, k, res)) { rc = MC_ESTATE; break; }
                if (res) bits[i] |= 1u << k;
            }
        }
        if (rc) { free(table); return rc; }
        const bool term = kind < 0;
        const LiveCheck ck{term ? LIVE_STABLE : kind, p, q};
        const uint64_t all = live_all_conjuncts(fu.nconj), weak = fu.weak_mask, strong = fu.strong_mask;
        const uint64_t *of_unit = fu.of_unit;
        auto in_m = [&](uint32_t d) { return term || live_in_mask(ck, bits[d]); };
        auto target = [&](uint32_t d) { return term ? !done[d] : live_in_target(ck, bits[d]); };
        memset(counts, 0, 8 * sizeof(uint64_t));
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
                live_state_masked_units((uint32_t)i, dst.data() + off[i], unit.data() + off[i], off[i + 1] - off[i], comp.data(), of_unit, [&](uint32_t d) { return keep[d] != 0; }, &en, &taken);
                en_of[i] = live_enabled_in_units((uint32_t)i, dst.data() + off[i], unit.data() + off[i], off[i + 1] - off[i], comp.data(), of_unit);
                live_merge(entry[comp[i]], taken, live_disabled(all, en), target((uint32_t)i));
                enabled[comp[i]] |= en_of[i];
            }
            bool still = false;
            for (size_t i = 0; i < n; i++) {
                if (!keep[i]) continue;
                const LiveComp &c = entry[comp[i]];
                const int cls = live_classify(all, weak, strong, c.taken, c.disabled, enabled[comp[i]], c.done, c.size);
                if (comp[i] == i && cls == LIVE_FINAL) {
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
        counts[2] = first_root;
        counts[5] = term ? (counts[1] ? 1 : 0) : 0;
        if (!term) {
            auto passable = [&](uint32_t d) { return live_passable(ck, bits[d]); };
            for (bool changed = true; changed;) {
                changed = false;
                for (size_t i = 0; i < n; i++) {
                    if (!passable((uint32_t)i) || dist[i] == 0) continue;
                    const uint32_t best = live_reach_step((uint32_t)i, dist[i], dst.data() + off[i], off[i + 1] - off[i], dist.data(), passable);
                    if (best < dist[i]) { dist[i] = best; changed = true; }
                }
            }
            for (size_t i = 0; i < n; i++)
                if (in_m((uint32_t)i) && dist[i] != LIVE_FAR && live_in_start(ck, bits[i], i < ninit)) counts[5] = 1;
        }
        FILE *fs = fopen(states_path, "w"), *fo = fopen(out_path, "w"), *fe = fopen(edges_path, "w");
        if (!fs || !fo || !fe) rc = -5;
        std::vector<char> txt(1 << 16);
        for (size_t i = 0; i < n && !rc; i++) {
            const int m = S::format(prm, &rows[i * W], txt.data(), txt.size());
            for (int k = 0; k < m; k++) if (txt[k] == '\n') txt[k] = ' ';
            fprintf(fs, "%.*s\n", m, txt.data());
            fprintf(fo, "%u %d\n", ids[i], (int)open[i]);
            for (uint64_t e = off[i]; e < off[i + 1]; e++)
                fprintf(fe, "%zu %u %d %llx\n", i, dst[e], (int)unit[e], (unsigned long long)live_conjuncts(of_unit, unit[e]));
        }
        if (fs) fclose(fs);
        if (fo) fclose(fo);
        if (fe) fclose(fe);
        free(table);
        return rc;
    }
}

extern "C" int unitshim_check(const mc_spec_desc *d, const mc_fair_units *fu, int kind, int p, int q, const char *states_path, const char *out_path,
                              const char *edges_path, uint64_t *counts) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) { return check<decltype(spec)>(prm, *fu, kind, p, q, states_path, out_path, edges_path, counts); });
}
