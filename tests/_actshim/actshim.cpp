// tests/_actshim/actshim.cpp — TEST-ONLY host search over the interpreter of compiled PlusCal programs (SpecVmCfg, spec_vm_cfg.h) that keeps
// what tests/_shim's does not: the (parent, slot) record of every stored state, so that the behaviour of the first violation — the engine's
// least (state, slot) key of the level — can be rebuilt and its LAST STEP handed out as text; and, with cont = 1, what -continue collects
// through the overloads of violations.h that take the model's number of invariants (viol_pair / viol_stored_bin with ninv).  g++, no HIP;
// the front end's host side comes from tests/_shim's library.
#include "pcal.h"
#include "violations.h"

#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

using namespace mc;

extern "C" {

#ifdef ACTSHIM_OWN_FRONT_END
// what the front end reports through: only the library built with a front end of its own defines it.  The other one is linked against
// tests/_shim's library and must leave that library's definition alone (a definition here would come first in the scope the dynamic
// linker gives the dependency, and tests/_shim's error texts would be lost for the whole process)
void mc_set_error_internal(const char *) {}
#endif

struct ActOut {
    uint64_t distinct, generated;
    uint32_t depth, trace_len;
    int32_t verdict, violated;        // MC_V_* / the invariant index of the first violation (least (state, slot) key of its level)
    uint32_t fatal, fatal_inv;        // cont: a pair ended the search; the index its status carried
    uint64_t fatal_pairs;
    uint64_t states[VIOL_BINS], outside[VIOL_BINS];
    uint64_t levels[256];
};

// before / after: the last two states of the first violation's behaviour (after = before for a behaviour of one state)
int actshim_search(const int64_t *params, unsigned np, int cont, ActOut *o, char *before, char *after, size_t cap) {
    using S = SpecVmCfg;
    VmParams prm;
    if (vm_make_params(params, np, prm)) return -1;
    memset(o, 0, sizeof *o);
    o->violated = -1;
    const int W = S::words(prm), ninv = ViolModel<S>::ninv(prm);
    std::vector<uint64_t> rows;
    std::vector<int64_t> parent;
    std::vector<int> pslot;
    std::unordered_set<uint64_t> seen;
    uint64_t tmp[S::MAX_WORDS];
    auto first = [&](int verdict, unsigned st, uint32_t len, const uint64_t *b, const uint64_t *a) {
        if (o->verdict) return;
        o->verdict = verdict;
        o->violated = verdict == MC_V_INVARIANT ? (int)(st >> 8 & 255) : -1;
        o->trace_len = len;
        if (before) S::format(prm, b, before, cap);
        if (after) S::format(prm, a, after, cap);
    };
    auto store = [&](const uint64_t *w, int64_t p, int slot) {
        rows.insert(rows.end(), w, w + W);
        parent.push_back(p);
        pslot.push_back(slot);
    };
    bool stop = false;
    for (uint64_t k = 0; k < S::num_init(prm); k++) {
        S::init(prm, k, WordRef{tmp, 1});
        o->generated++;
        const unsigned st = S::init_status(prm, CWordRef{tmp, 1});
        if (st & ST_SPECERR) first(MC_V_SPECERR, st, 1, tmp, tmp);
        else if (st & ST_INVARIANT) first(MC_V_INVARIANT, st, 1, tmp, tmp);
        if (st & ST_OUT_OF_MODEL) continue;
        if (seen.insert(S::fp_of(prm, CWordRef{tmp, 1})).second) store(tmp, -1, -1);
    }
    size_t lo = 0, hi = parent.size();
    uint32_t level = 1;
    o->levels[0] = hi;
    auto stored_pass = [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            const CWordRef self{&rows[i * (size_t)W], 1};
            const int bin = viol_stored_bin<S>(prm, self, parent[i] >= 0, ninv, []() { return 0u; }, [&]() {
                const CWordRef ps{&rows[(size_t)parent[i] * (size_t)W], 1};
                S::Local loc;
                S::load(prm, ps, loc);
                uint64_t f = 0;
                return S::eval(prm, loc, ps, pslot[i], f);
            });
            if (bin >= 0) o->states[bin]++;
        }
    };
    if (o->verdict) { if (cont) stored_pass(0, hi); if (!cont) stop = true; }
    while (lo < hi && !stop && level < 255) {
        for (size_t i = lo; i < hi; i++) {
            const std::vector<uint64_t> cur(rows.begin() + (long)(i * (size_t)W), rows.begin() + (long)((i + 1) * (size_t)W));
            const CWordRef s{cur.data(), 1};
            S::Local loc;
            S::load(prm, s, loc);
            for (int slot = 0; slot < S::nslots(prm, loc); slot++) {
                uint64_t fp = 0;
                const unsigned st = S::eval(prm, loc, s, slot, fp);
                if (!(st & ST_ENABLED)) continue;
                o->generated++;
                S::apply(prm, s, slot, WordRef{tmp, 1});
                if (st & ST_ASSERT) first(MC_V_ASSERT, st, level, cur.data(), cur.data());
                else if (st & ST_SPECERR) first(MC_V_SPECERR, st, level, cur.data(), cur.data());
                else if (st & ST_INVARIANT) first(MC_V_INVARIANT, st, level + 1, cur.data(), tmp);
                if (cont) {
                    const ViolPair r = viol_pair<S>(st, ninv);
                    if (viol_pair_column(r) == 1) o->outside[r.bin]++;
                    if (viol_ends_search(r)) { o->fatal_pairs++; if (!o->fatal) { o->fatal = 1; o->fatal_inv = r.inv; } }
                }
                if (st & (ST_ASSERT | ST_SPECERR | ST_OUT_OF_MODEL)) continue;
                if (seen.insert(fp).second) store(tmp, (int64_t)i, slot);
            }
        }
        if (cont && o->verdict) stored_pass(hi, parent.size());
        if (cont ? o->fatal != 0 : o->verdict != 0) stop = true;
        lo = hi;
        hi = parent.size();
        if (lo < hi) o->levels[level++] = hi - lo;
    }
    o->distinct = parent.size();
    o->depth = level;
    return 0;
}

// the front end of the library this one is linked against (a mutant's, in the mutation test): names separated by blanks; NULL = refused
void *actshim_compile(const char *tla, const char *properties, const char *invariants, const char *action_constraints) {
    auto names = [](const char *s) {
        std::vector<std::string> out;
        std::string cur;
        for (const char *p = s ? s : ""; ; p++) {
            if (*p && *p != ' ') { cur += *p; continue; }
            if (!cur.empty()) out.push_back(cur);
            cur.clear();
            if (!*p) break;
        }
        return out;
    };
    pcal::Config cf;
    cf.properties = names(properties);
    cf.invariants = names(invariants);
    cf.action_constraints = names(action_constraints);
    pcal::Module m;
    const std::string text(tla);
    if (!pcal::parse_module(text, m).empty()) return nullptr;
    auto *p = new pcal::Program();
    if (!pcal::compile(m, text, cf, *p).empty()) { delete p; return nullptr; }
    return p;
}
void actshim_free(void *p) { delete (pcal::Program *)p; }

// the two rules on a bare status word, for the cases no small model reaches
void actshim_pair(unsigned st, int ninv, unsigned *what, unsigned *bin, unsigned *inv) {
    const ViolPair r = viol_pair<SpecVmCfg>(st, ninv);
    *what = r.what; *bin = r.bin; *inv = r.inv;
}
int actshim_stored_bin(unsigned st, int ninv) {
    VmParams prm;
    memset(&prm, 0, sizeof prm);
    return viol_stored_bin<SpecVmCfg>(prm, CWordRef{nullptr, 1}, true, ninv, []() { return 0u; }, [&]() { return st; });
}

}  // extern "C"
