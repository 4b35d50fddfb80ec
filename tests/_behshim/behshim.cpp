// tests/_behshim/behshim.cpp — TEST-ONLY host build of the behaviour rule (tla_rust_amd/csrc/behaviour.h) over the spec lowerings, with
// g++ and no HIP: the very beh_check that mc_engine_behaviour_witness runs and that the device kernel k_behaviours must reproduce field
// for field.  tests/test_behaviours_host.py checks it against a plain reference over the oracle's state graph (tests/behaviours.py);
// tests/test_gpu_behaviours.py checks the device against it.  Linked against tests/_shim's libshim.so for the PlusCal front-end
// (vm_make_params and friends), like tests/_simshim.
#include "spec_registry.h"   // -I <a csrc directory>: the product's, or a copy with one line of behaviour.h edited (the mutants)
#include "behaviour.h"
#include <string.h>
#include <vector>

using namespace mc;

extern "C" int behshim_words(const mc_spec_desc *d) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) { return decltype(spec)::words(prm); });
}
extern "C" int behshim_format(const mc_spec_desc *d, const uint64_t *row, char *buf, size_t cap) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) { return decltype(spec)::format(prm, row, buf, cap); });
}
// the batch: out[b] for every behaviour
extern "C" int behshim_check(const mc_spec_desc *d, uint64_t count, const uint64_t *first, const uint64_t *rows, const uint64_t *mask, unsigned flags,
                             mc_beh_verdict *out) {
    return dispatch_spec(d, [&](auto spec, const auto &prm) {
        using S = decltype(spec);
        const int W = S::words(prm);
        for (uint64_t b = 0; b < count; ++b)
            if (int rc = beh_check<S>(prm, rows + first[b] * W, first[b + 1] - first[b], mask, flags, &out[b], nullptr)) return rc;
        return 0;
    });
}
// one behaviour with everything it built: sizes[i] = |K_i| for the sets built (returns how many), their rows one set after the other
// into set_rows (capacity cap_rows rows; -1 when too small); witness rows / slots as mc_engine_behaviour_witness gives them
extern "C" long behshim_sets(const mc_spec_desc *d, const uint64_t *rows, uint64_t T, const uint64_t *mask, unsigned flags, mc_beh_verdict *out,
                             uint32_t *sizes, uint64_t *set_rows, size_t cap_rows, uint64_t *wit_rows, int32_t *wit_slots) {
    long n = -1;
    dispatch_spec(d, [&](auto spec, const auto &prm) {
        using S = decltype(spec);
        const int W = S::words(prm);
        BehSets bs;
        beh_check<S>(prm, rows, T, mask, flags, out, &bs);
        size_t at = 0;
        for (size_t i = 0; i < bs.sets.size(); ++i) {
            sizes[i] = (uint32_t)bs.sets[i].size();
            for (const auto &m : bs.sets[i]) {
                if (at == cap_rows) return 0;
                memcpy(set_rows + at++ * W, m.row.data(), W * sizeof(uint64_t));
            }
        }
        if (wit_rows) beh_witness(bs, W, wit_rows, wit_slots);
        n = (long)bs.sets.size();
        return 0;
    });
    return n;
}
// the model's graph as the lowering gives it, for building test inputs: initial state k (returns num_init), and the successor of `row`
// through `slot` (returns the ST_* status word, 0 = not enabled; *nslots = the row's slot count)
extern "C" long behshim_init(const mc_spec_desc *d, uint64_t k, uint64_t *row) {
    long n = -1;
    dispatch_spec(d, [&](auto spec, const auto &prm) {
        using S = decltype(spec);
        n = (long)S::num_init(prm);
        if (k < (uint64_t)n) S::init(prm, k, WordRef{row, 1});
        return 0;
    });
    return n;
}
extern "C" unsigned behshim_succ(const mc_spec_desc *d, const uint64_t *row, int slot, uint64_t *succ, int *nslots) {
    unsigned st = 0;
    dispatch_spec(d, [&](auto spec, const auto &prm) {
        using S = decltype(spec);
        const int W = S::words(prm);
        typename S::Local loc;
        const CWordRef s{row, 1};
        S::load(prm, s, loc);
        *nslots = S::nslots(prm, loc);
        if (slot < 0 || slot >= *nslots) return 0;
        uint64_t f = 0;
        st = S::eval(prm, loc, s, slot, f);
        if (beh_step_kind(st) == BEH_STEP || beh_step_kind(st) == BEH_STEP_OUTSIDE) {
            if (st & ST_SELFLOOP) memcpy(succ, row, W * sizeof(uint64_t));
            else S::apply(prm, s, slot, WordRef{succ, 1});
        }
        return 0;
    });
    return st;
}
