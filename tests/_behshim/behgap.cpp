// tests/_behshim/behgap.cpp — TEST-ONLY host build (g++, no HIP) of what behaviour checking with unlogged steps adds to
// tla_rust_amd/csrc/behaviour.h: the rule over the test lowering SpecGap (behgap.h; tests/test_behaviours_hidden_host.py holds the
// cases of tests/test_gpu_behaviours_hidden.py against hand-computed figures without a GPU), and beh_path — what
// mc_engine_behaviour_path returns — over the spec lowerings.  Linked against tests/_shim's libshim.so like behshim.cpp.
#include "behgap.h"   // -I <a csrc directory>: the product's, or a copy with one line of behaviour.h edited (the mutants)
#include <string.h>

using namespace mc;

extern "C" int bg_host(uint64_t K, uint64_t h0, int G, int B, int on, uint64_t count, const uint64_t *first, const uint64_t *rows, const uint64_t *mask,
                       unsigned flags, mc_beh_verdict *out) {
    return gap_host(SpecGap::Params{K, h0, G, B, on, 0}, count, first, rows, mask, flags, out);
}

template <class S>
static long path_of(const typename S::Params &prm, const uint64_t *rows, uint64_t T, const uint64_t *mask, unsigned flags, mc_beh_verdict *out,
                    uint64_t *states, int32_t *slots, uint32_t *obs, size_t cap) {
    const int W = S::words(prm);
    BehSets bs;
    beh_check<S>(prm, rows, T, mask, flags, out, &bs);
    const BehPath p = beh_path(bs, W);
    if (p.slots.size() > cap) return -1;
    memcpy(states, p.states.data(), p.states.size() * sizeof(uint64_t));
    memcpy(slots, p.slots.data(), p.slots.size() * sizeof(int32_t));
    memcpy(obs, p.obs.data(), p.obs.size() * sizeof(uint32_t));
    return (long)p.slots.size();
}
// one behaviour's verdict and its path with the hidden states in it: returns the number of states (-1: cap too small)
extern "C" long behgap_path(const mc_spec_desc *d, const uint64_t *rows, uint64_t T, const uint64_t *mask, unsigned flags, mc_beh_verdict *out,
                            uint64_t *states, int32_t *slots, uint32_t *obs, size_t cap) {
    long n = -1;
    dispatch_spec(d, [&](auto spec, const auto &prm) {
        n = path_of<decltype(spec)>(prm, rows, T, mask, flags, out, states, slots, obs, cap);
        return 0;
    });
    return n;
}
// how wide the closures of a batch are: the sum of |C| over every observation i >= 1 that was enumerated, and how many those are
extern "C" int behgap_closure_sizes(const mc_spec_desc *d, uint64_t count, const uint64_t *first, const uint64_t *rows, const uint64_t *mask,
                                    unsigned flags, uint64_t *sum_out, uint64_t *n_out) {
    *sum_out = *n_out = 0;
    return dispatch_spec(d, [&](auto spec, const auto &prm) {
        using S = decltype(spec);
        const int W = S::words(prm);
        for (uint64_t b = 0; b < count; ++b) {
            BehSets bs;
            mc_beh_verdict v;
            beh_check<S>(prm, rows + first[b] * W, first[b + 1] - first[b], mask, flags, &v, &bs);
            for (size_t i = 1; i < bs.closures.size(); ++i) { *sum_out += bs.closures[i].size(); ++*n_out; }
        }
        return 0;
    });
}
extern "C" long bg_path(uint64_t K, uint64_t h0, int G, int B, int on, const uint64_t *rows, uint64_t T, const uint64_t *mask, unsigned flags,
                        mc_beh_verdict *out, uint64_t *states, int32_t *slots, uint32_t *obs, size_t cap) {
    return path_of<SpecGap>(SpecGap::Params{K, h0, G, B, on, 0}, rows, T, mask, flags, out, states, slots, obs, cap);
}
