// tests/_graphshim/graphshim.cpp — TEST-ONLY host build of what the state graph is made of (tla_rust_amd/csrc/graph.h: seen_find,
// graph_edge, graph_state) over the spec lowerings, with g++ and no HIP: the very lookup and edge rule the device kernels of
// engine_graph.h run.  A plain sequential search of the whole state graph (no stop at a violation, like the oracle's graph dump) inserts
// its fingerprints into a table IN THE SEEN-SET'S LAYOUT — buckets of 8 or MC_SPARSE_SLOTS slots, home bucket from the low 32 bits,
// the slot order rotated by bits 32.., linear probing with wrap-around: restated here from the comment above seen_insert_t — sized by
// the caller, so that a test can make lookups leave the home bucket.  Then graph.h walks every stored state over that table.
//
// tests/test_graph_host.py compares the edge multiset with the oracle's edge file by state TEXT.  Linked against tests/_shim's
// libshim.so (the host helpers of compiled programs), like tests/_covshim.
#include "spec_registry.h"   // -I <a csrc directory>: the product's, or a copy with one edit (the mutants of tests/test_graph_host.py)
#include "graph.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace mc;

// the slot a NEW key takes (or the one that holds it already); ~0 = the table is full.  *fresh: the key was not there.
template <int SLOTS>
static uint64_t host_insert(uint64_t *table, uint64_t nbuckets, uint64_t fp, bool *fresh) {
    uint64_t bk = ((fp & 0xffffffffull) * nbuckets) >> 32;
    const unsigned j0 = (unsigned)(fp >> 32) & (unsigned)(SLOTS - 1);
    for (uint64_t probe = 0; probe < 2048 && probe < nbuckets; ++probe) {
        for (int i = 0; i < SLOTS; i++)
            if (table[bk * SLOTS + i] == fp) { *fresh = false; return bk * SLOTS + i; }
        for (unsigned r = 0; r < (unsigned)SLOTS; r++) {
            const unsigned i = (j0 + r) & (unsigned)(SLOTS - 1);
            if (table[bk * SLOTS + i] == 0) { table[bk * SLOTS + i] = fp; *fresh = true; return bk * SLOTS + i; }
        }
        bk = bk + 1 == nbuckets ? 0 : bk + 1;
    }
    return ~0ull;
}

// states_path: one line "L<level> <state text>" per stored state, in the order found (line k = state k);
// edges_path: one line "<source state> <action id> <destination state>" per edge, rows in state order, a row in slot order.
// counts: [0] states, [1] edges, [2] self loops, [3] dropped, [4] missing, [5] lookups that left their home bucket, [6] generated
template <class S>
static int search(const typename S::Params &prm, uint64_t nbuckets, int sparse, const char *states_path, const char *edges_path, uint64_t *counts) {
    const int W = S::words(prm);
    const int SL = sparse ? MC_SPARSE_SLOTS : 8;
    const uint64_t seen = sparse ? (nbuckets | GRAPH_SEEN_SPARSE) : nbuckets;
    uint64_t *table = (uint64_t *)aligned_alloc(64, (size_t)nbuckets * SL * sizeof(uint64_t));   // (graph.h reads buckets with aligned loads)
    if (!table) return -4;
    memset(table, 0, (size_t)nbuckets * SL * sizeof(uint64_t));
    std::vector<uint32_t> slot_index((size_t)nbuckets * SL, 0xffffffffu);
    std::vector<uint64_t> rows;      // every stored state, W words each
    std::vector<unsigned> level;
    memset(counts, 0, 7 * sizeof(uint64_t));
    int rc = 0;
    auto put = [&](uint64_t fp, const uint64_t *w, unsigned lv) {
        bool fresh = false;
        const uint64_t pos = sparse ? host_insert<MC_SPARSE_SLOTS>(table, nbuckets, fp, &fresh) : host_insert<8>(table, nbuckets, fp, &fresh);
        if (pos == ~0ull) { rc = MC_ETABLEFULL; return; }
        if (!fresh) return;
        slot_index[pos] = (uint32_t)level.size();
        rows.insert(rows.end(), w, w + W);
        level.push_back(lv);
    };
    uint64_t tmp[S::MAX_WORDS];
    for (uint64_t k = 0; k < S::num_init(prm) && !rc; k++) {
        S::init(prm, k, WordRef{tmp, 1});
        counts[6]++;
        if (S::init_status(prm, CWordRef{tmp, 1}) & ST_OUT_OF_MODEL) continue;
        put(S::fp_of(prm, CWordRef{tmp, 1}), tmp, 1);
    }
    for (size_t i = 0; i < level.size() && !rc; i++) {   // (rows grows while it is walked: index, not pointer)
        std::vector<uint64_t> cur(rows.begin() + i * W, rows.begin() + (i + 1) * W);
        const CWordRef s{cur.data(), 1};
        typename S::Local loc;
        S::load(prm, s, loc);
        const int ns = S::nslots(prm, loc);
        for (int slot = 0; slot < ns && !rc; slot++) {
            uint64_t fp = 0;
            const unsigned st = S::eval(prm, loc, s, slot, fp);
            if (!(st & ST_ENABLED)) continue;
            counts[6]++;
            if (st & ST_OVERFLOW) { rc = MC_EOVERFLOW; break; }
            if (st & (ST_ASSERT | ST_SPECERR | ST_OUT_OF_MODEL | ST_SELFLOOP)) continue;
            S::apply(prm, s, slot, WordRef{tmp, 1});
            put(fp, tmp, level[i] + 1);
        }
    }
    FILE *fs = rc ? nullptr : fopen(states_path, "w"), *fe = rc ? nullptr : fopen(edges_path, "w");
    if (!rc && (!fs || !fe)) rc = -5;
    std::vector<char> txt(1 << 16);
    for (size_t i = 0; i < level.size() && !rc; i++) {
        const uint64_t *w = &rows[i * W];
        const int m = S::format(prm, w, txt.data(), txt.size());
        for (int k = 0; k < m; k++) if (txt[k] == '\n') txt[k] = ' ';
        fprintf(fs, "L%u %.*s\n", level[i], m, txt.data());
        // every stored state's own key is found where the search put it (k_graph_index's lookup)
        const uint64_t own = seen_find(table, seen, S::fp_of(prm, CWordRef{w, 1}));
        if (own == GRAPH_ABSENT || slot_index[own] != (uint32_t)i) { counts[4]++; continue; }
        const uint64_t fpw = S::fp_of(prm, CWordRef{w, 1});
        if (own / SL != (((fpw & 0xffffffffull) * nbuckets) >> 32)) counts[5]++;
        graph_state<S>(prm, CWordRef{w, 1}, table, seen, [&](unsigned kind, uint64_t pos, int action, int) {
            if (kind == GE_DROPPED) { counts[3]++; return; }
            if (kind == GE_MISSING || (kind == GE_EDGE && slot_index[pos] == 0xffffffffu)) { counts[4]++; return; }
            const uint32_t to = kind == GE_SELF ? (uint32_t)i : slot_index[pos];
            counts[1]++;
            counts[2] += to == (uint32_t)i ? 1 : 0;
            fprintf(fe, "%zu %d %u\n", i, action, to);
        });
    }
    if (fs) fclose(fs);
    if (fe) fclose(fe);
    free(table);
    counts[0] = level.size();
    return rc;
}

extern "C" int graphshim_search(const mc_spec_desc *d, uint64_t nbuckets, int sparse, const char *states_path, const char *edges_path, uint64_t *counts) {
    if (!nbuckets) return MC_EBADCFG;
    return dispatch_spec(d, [&](auto spec, const auto &prm) { return search<decltype(spec)>(prm, nbuckets, sparse, states_path, edges_path, counts); });
}
extern "C" const char *graphshim_action_name(const mc_spec_desc *d, int action) {
    const char *nm = "?";
    dispatch_spec(d, [&](auto spec, const auto &prm) {
        if constexpr (std::is_same_v<std::decay_t<decltype(prm)>, VmParams>) nm = vm_action_name(prm.host, action);
        else nm = decltype(spec)::action_name(action);
        return 0;
    });
    return nm;
}
