// tests/_livepropshim/livepropshim.cpp — TEST-ONLY host build of the rule by which <>Q, []<>Q, <>[]P and P ~> Q are decided
// (tla_rust_amd/csrc/liveness.h: LivePred, live_in_mask / live_in_start / live_in_target, live_own_component, live_state_masked,
// live_merge, live_violates_masked, live_passable, live_reach_step) over the compiled-program lowering, with g++ and no HIP: the very
// functions the device kernels of engine_live.h and engine_graph.h call.  As tests/_liveshim does, a plain sequential search fills a
// table in the seen-set's layout, graph.h gives every state's row and LiveProc the process of every edge.  What the device does in
// parallel is sequential here: the components of the masked graph come from a Tarjan over the edges between states that are no
// component of their own, the reach pass sweeps the states in index order until nothing changes.
//
// tests/test_liveprops_host.py compares the predicate bits, the violating components and the witness with tests/liveprops.py by state
// TEXT, and builds this file against copies of csrc with one edit each (the mutants).  Linked against tests/_shim's libshim.so.
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

// states_path: one line per state, its text; out_path: one line per state "<predicate bits> <component id in the masked graph> <1 when
// that component is judged violating> <dist, -1 = none>".  counts: [0] states, [1] violating components, [2] the witness (~0 = none),
// [3] predicates, [4] states in M, [5] bad starts
template <class S>
static int check(const typename S::Params &prm, uint64_t fair, int kind, int p, int q, const char *states_path, const char *out_path, uint64_t *counts) {
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
        const LiveCheck ck{kind, p, q};
        // ---- the components of the masked graph
        std::vector<char> keep(n);
        for (size_t i = 0; i < n; i++) keep[i] = !live_own_component(ck, bits[i]);
        std::vector<uint32_t> comp;
        tarjan(off, dst, keep, comp);
        // ---- the rule per component: only states of M are merged and judged
        const int np = LiveProc<S>::count(prm);
        const uint64_t all = np >= 64 ? ~0ull : (1ull << np) - 1;
        std::vector<LiveComp> entry(n);
        auto in_m = [&](uint32_t d) { return live_in_mask(ck, bits[d]); };
        for (size_t i = 0; i < n; i++) {
            if (!in_m((uint32_t)i)) continue;
            uint64_t en = 0, taken = 0;
            live_state_masked((uint32_t)i, dst.data() + off[i], proc.data() + off[i], off[i + 1] - off[i], comp.data(), in_m, &en, &taken);
            live_merge(entry[comp[i]], taken, live_disabled(all, en), live_in_target(ck, bits[i]));
        }
        std::vector<char> bad(n, 0);
        std::vector<uint32_t> dist(n, LIVE_FAR);
        memset(counts, 0, 6 * sizeof(uint64_t));
        for (size_t i = 0; i < n; i++) {
            const LiveComp &c = entry[comp[i]];
            bad[i] = in_m((uint32_t)i) && live_violates_masked(all, fair, c.taken, c.disabled, c.done, c.size);
            if (bad[i]) dist[i] = 0;
            if (bad[i] && comp[i] == i) counts[1]++;
            if (in_m((uint32_t)i)) counts[4]++;
        }
        // ---- reach, to a fixed point
        auto passable = [&](uint32_t d) { return live_passable(ck, bits[d]); };
        for (bool changed = true; changed;) {
            changed = false;
            for (size_t i = 0; i < n; i++) {
                if (!passable((uint32_t)i) || dist[i] == 0) continue;
                const uint32_t best = live_reach_step((uint32_t)i, dist[i], dst.data() + off[i], off[i + 1] - off[i], dist.data(), passable);
                if (best < dist[i]) { dist[i] = best; changed = true; }
            }
        }
        counts[0] = n;
        counts[2] = ~0ull;
        counts[3] = (uint64_t)tab.n;
        for (size_t i = n; i-- > 0;)
            if (in_m((uint32_t)i) && dist[i] != LIVE_FAR && live_in_start(ck, bits[i], i < ninit)) { counts[2] = i; counts[5]++; }
        FILE *fs = fopen(states_path, "w"), *fo = fopen(out_path, "w");
        if (!fs || !fo) rc = -5;
        std::vector<char> txt(1 << 16);
        for (size_t i = 0; i < n && !rc; i++) {
            const int m = S::format(prm, &rows[i * W], txt.data(), txt.size());
            for (int k = 0; k < m; k++) if (txt[k] == '\n') txt[k] = ' ';
            fprintf(fs, "%.*s\n", m, txt.data());
            fprintf(fo, "%u %u %d %lld\n", bits[i], comp[i], bad[i] ? 1 : 0, dist[i] == LIVE_FAR ? -1ll : (long long)dist[i]);
        }
        if (fs) fclose(fs);
        if (fo) fclose(fo);
        free(table);
        return rc;
    }
}

extern "C" int livepropshim_check(const mc_spec_desc *d, uint64_t fair, int kind, int p, int q, const char *states_path, const char *out_path, uint64_t *counts) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) { return check<decltype(spec)>(prm, fair, kind, p, q, states_path, out_path, counts); });
}

// What a cfg without such a property must leave untouched: the program image and the scalar fields of VmParams (the pointers left out),
// as the engine reads them.  Returns the image's length in words; at most cap of them go to image_out.  fields_out: 22 values.
extern "C" long livepropshim_image(const mc_spec_desc *d, int32_t *image_out, size_t cap, int64_t *fields_out) {
    VmParams p;
    if (vm_make_params(d->params, d->nparams, p)) return -1;
    const int f[] = {p.nv, p.words, p.ninst, p.maxch, p.pc_base, p.done, p.init_entry, p.ninv, p.ncon, p.label_tab, p.self_tab, p.code_len};
    for (int k = 0; k < 12; k++) fields_out[k] = f[k];
    for (int k = 0; k < 8; k++) fields_out[12 + k] = p.inv_entry[k];
    fields_out[20] = (int64_t)p.num_init;
    fields_out[21] = (int64_t)sizeof(VmParams);
    for (int k = 0; k < p.code_len && (size_t)k < cap; k++) image_out[k] = p.code[k];
    return p.code_len;
}
