// tests/_liveshim/liveshim.cpp — TEST-ONLY host build of the rule `Termination` is decided by (tla_rust_amd/csrc/liveness.h: LiveProc,
// live_real_step, live_state, live_merge, live_fair, live_violates) over the compiled-program lowering, with g++ and no HIP: the very
// functions the device kernels of engine_live.h call.  A plain sequential search of the whole state graph fills a table in the seen-set's
// layout (as tests/_graphshim does), graph.h gives every state's row, LiveProc the process of every edge; the components come from a
// sequential Tarjan written here (the device's trimming and colouring are checked against another Tarjan on the GPU).
//
// tests/test_liveness_host.py compares the components and the fair non-Done ones with tests/livegraph.py by state TEXT, and builds this
// file against copies of csrc with one edit each (the mutants).  Linked against tests/_shim's libshim.so, like tests/_graphshim.
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

// comp[v] = the least vertex of v's component (iterative Tarjan over CSR rows)
static void tarjan(const std::vector<uint64_t> &off, const std::vector<uint32_t> &dst, std::vector<uint32_t> &comp) {
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

// states_path: one line per state, its text; out_path: one line per state "<component id> <1 when the component is fair and holds no
// Done state>".  counts: [0] states, [1] components, [2] fair non-Done components, [3] process instances
template <class S>
static int check(const typename S::Params &prm, uint64_t fair, const char *states_path, const char *out_path, uint64_t *counts) {
    if constexpr (!LiveProc<S>::HAS) {
        return MC_ENOSPEC;
    } else {
        const int W = S::words(prm);
        const uint64_t nbuckets = 1 << 13, seen = nbuckets;
        uint64_t *table = (uint64_t *)aligned_alloc(64, (size_t)nbuckets * 8 * sizeof(uint64_t));
        if (!table) return -4;
        memset(table, 0, (size_t)nbuckets * 8 * sizeof(uint64_t));
        std::vector<uint32_t> slot_index((size_t)nbuckets * 8, 0xffffffffu);
        std::vector<uint64_t> rows;
        size_t n = 0;
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
        // rows of the graph, with the process of every edge
        std::vector<uint64_t> off(n + 1, 0);
        std::vector<uint32_t> dst;
        std::vector<int8_t> proc;
        for (size_t i = 0; i < n && !rc; i++) {
            graph_state<S>(prm, CWordRef{&rows[i * W], 1}, table, seen, [&](unsigned kind, uint64_t pos, int, int slot) {
                if (kind != GE_SELF && kind != GE_EDGE) return;
                const uint32_t to = kind == GE_SELF ? (uint32_t)i : slot_index[pos];
                if (to == 0xffffffffu) { rc = MC_ESTATE; return; }
                dst.push_back(to);
                proc.push_back((int8_t)LiveProc<S>::of(prm, slot));
            });
            off[i + 1] = dst.size();
        }
        if (rc) { free(table); return rc; }
        std::vector<uint32_t> comp;
        tarjan(off, dst, comp);
        const int np = LiveProc<S>::count(prm);
        const uint64_t all = np >= 64 ? ~0ull : (1ull << np) - 1;
        std::vector<LiveComp> entry(n);
        for (size_t i = 0; i < n; i++) {
            uint64_t en = 0, taken = 0;
            bool done = false;
            live_state((uint32_t)i, dst.data() + off[i], proc.data() + off[i], off[i + 1] - off[i], comp.data(), &en, &taken, &done);
            live_merge(entry[comp[i]], taken, live_disabled(all, en), done);
        }
        memset(counts, 0, 4 * sizeof(uint64_t));
        counts[0] = n;
        counts[3] = (uint64_t)np;
        FILE *fs = fopen(states_path, "w"), *fo = fopen(out_path, "w");
        if (!fs || !fo) rc = -5;
        std::vector<char> txt(1 << 16);
        for (size_t i = 0; i < n && !rc; i++) {
            const int m = S::format(prm, &rows[i * W], txt.data(), txt.size());
            for (int k = 0; k < m; k++) if (txt[k] == '\n') txt[k] = ' ';
            fprintf(fs, "%.*s\n", m, txt.data());
            const LiveComp &c = entry[comp[i]];
            const bool bad = live_violates(all, fair, c.taken, c.disabled, c.done, c.size);
            if (comp[i] == i) { counts[1]++; counts[2] += bad ? 1 : 0; }
            fprintf(fo, "%u %d\n", comp[i], bad ? 1 : 0);
        }
        if (fs) fclose(fs);
        if (fo) fclose(fo);
        free(table);
        return rc;
    }
}

extern "C" int liveshim_check(const mc_spec_desc *d, uint64_t fair, const char *states_path, const char *out_path, uint64_t *counts) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) { return check<decltype(spec)>(prm, fair, states_path, out_path, counts); });
}
