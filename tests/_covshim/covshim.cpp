// tests/_covshim/covshim.cpp — TEST-ONLY host build of what -coverage counts (tla_rust_amd/csrc/coverage.h: cov_counts, CovAction<S>,
// cov_state) over the spec lowerings, with g++ and no HIP: the very classification and action mapping the device kernels of
// engine_coverage.h run, driven by a plain sequential search of the whole state graph (no stop at a violation, like the oracle's graph
// dump: flagged and out-of-model successors are generated, never stored).
//
// tests/test_coverage_host.py compares the per-action sums with the oracle's edge file, action name by action name, and the states
// searched with the oracle's dump.  Linked against tests/_shim's libshim.so (the host helpers of compiled programs), like tests/_simshim.
#include "spec_registry.h"   // -I <a csrc directory>: the product's, or a copy with one edit (the mutants of tests/test_coverage_host.py)
#include "coverage.h"
#include <stdio.h>
#include <string.h>
#include <string>
#include <unordered_set>
#include <vector>

using namespace mc;

// generated / distinct: [COV_MAX_BINS], bin 0 = Init, bin a + 1 = action id a (distinct: the action of the pair that found the state
// first in this search's order); dump_path: one line "L<level> <state text>" per stored state, in the order found
template <class S>
static int search(const typename S::Params &prm, const char *dump_path, uint64_t *generated, uint64_t *distinct, int *nbins, uint64_t *nstates) {
    const int W = S::words(prm);
    *nbins = CovAction<S>::nbins(prm);
    if (*nbins > COV_MAX_BINS) return -2;
    memset(generated, 0, sizeof(uint64_t) * COV_MAX_BINS);
    memset(distinct, 0, sizeof(uint64_t) * COV_MAX_BINS);
    FILE *dump = dump_path ? fopen(dump_path, "w") : nullptr;
    std::vector<char> txt(1 << 16);
    std::unordered_set<uint64_t> seen;
    std::vector<uint64_t> cur, next;
    uint64_t n = 0;
    auto store = [&](const uint64_t *w, unsigned level, int bin) {
        next.insert(next.end(), w, w + W);
        distinct[bin]++;
        n++;
        if (dump) {
            const int m = S::format(prm, w, txt.data(), txt.size());
            for (int i = 0; i < m; i++) if (txt[i] == '\n') txt[i] = ' ';
            fprintf(dump, "L%u %.*s\n", level, m, txt.data());
        }
    };
    uint64_t tmp[S::MAX_WORDS];
    for (uint64_t k = 0; k < S::num_init(prm); k++) {
        S::init(prm, k, WordRef{tmp, 1});
        generated[0]++;
        const unsigned st = S::init_status(prm, CWordRef{tmp, 1});
        if (st & ST_OUT_OF_MODEL) continue;
        if (seen.insert(S::fp_of(prm, CWordRef{tmp, 1})).second) store(tmp, 1, 0);
    }
    int rc = 0;
    for (unsigned level = 1; !next.empty() && !rc; level++) {
        cur.swap(next);
        next.clear();
        for (size_t i = 0; i < cur.size() / (size_t)W && !rc; i++) {
            const CWordRef s{&cur[i * W], 1};
            // the counts: coverage.h's loop, as the device kernel runs it
            cov_state<S>(prm, s, [&](int a) { if (a + 1 >= 0 && a + 1 < *nbins) generated[a + 1]++; else rc = -3; });
            // the search itself (tests/_shim's)
            typename S::Local loc;
            S::load(prm, s, loc);
            const int ns = S::nslots(prm, loc);
            for (int slot = 0; slot < ns; slot++) {
                uint64_t fp = 0;
                const unsigned st = S::eval(prm, loc, s, slot, fp);
                if (!(st & ST_ENABLED)) continue;
                if (st & ST_OVERFLOW) { rc = MC_EOVERFLOW; break; }
                if (st & (ST_ASSERT | ST_SPECERR | ST_OUT_OF_MODEL | ST_SELFLOOP)) continue;
                if (seen.insert(fp).second) {
                    S::apply(prm, s, slot, WordRef{tmp, 1});
                    store(tmp, level + 1, CovAction<S>::of(prm, loc, s, slot) + 1);
                }
            }
        }
    }
    if (dump) fclose(dump);
    *nstates = n;
    return rc;
}

extern "C" int covshim_search(const mc_spec_desc *d, const char *dump_path, uint64_t *generated, uint64_t *distinct, int *nbins, uint64_t *nstates) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) { return search<decltype(spec)>(prm, dump_path, generated, distinct, nbins, nstates); });
}
extern "C" int covshim_listed(const mc_spec_desc *d, int action) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) { return CovAction<decltype(spec)>::listed(prm, action) ? 1 : 0; });
}
extern "C" const char *covshim_action_name(const mc_spec_desc *d, int action) {
    const char *nm = "?";
    dispatch_spec(d, [&](auto spec, const auto &prm) {
        if constexpr (std::is_same_v<std::decay_t<decltype(prm)>, VmParams>) nm = vm_action_name(prm.host, action);
        else nm = decltype(spec)::action_name(action);
        return 0;
    });
    return nm;
}
