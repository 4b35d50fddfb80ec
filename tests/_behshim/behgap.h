// tests/_behshim/behgap.h — TEST-ONLY lowering for behaviour checking with unlogged steps (MC_BEH_F_HIDDEN), shared by behgap.hip (the
// kernel k_behaviours<SpecGap, MUTANT, true>) and behgap.cpp (the host rule with g++).
//
// SpecGap: a row is two words, x (logged) and h (hidden).  num_init = K initial states (x = 0, h = h0 + k).  Slots:
//   0          tick   x' = x + 1, h' = 0        iff h == G
//   1          work   h' = h + 1                iff h < G
//   2          fold   h' = h / 2                (rows 2j and 2j + 1 have one successor: neighbouring lanes bring it in one depth)
//   3          spin   h' = h ^ 1                (a hidden two-cycle)
//   4 .. 3+B   fan_j  h' = h * B + j + 1000     (B fresh hidden rows per member: a closure that grows past 64)
//   4+B        leak   x' = x + 2, h kept        (an internal step that does touch the logged word)
// fold, spin and leak exist where the case's `on` has their bit (ON_FOLD / ON_SPIN / ON_LEAK); fan where B > 0.
#pragma once
#include "spec_registry.h"
#include "behaviour.h"

namespace mc {
struct SpecGap {
    enum : int { ON_FOLD = 1, ON_SPIN = 2, ON_LEAK = 4 };
    struct Params { uint64_t K, h0; int G, B, on, pad; };
    struct Local { uint64_t x, h; };
    static constexpr int MAX_WORDS = 2;
    MC_HD static int words(const Params &) { return 2; }
    MC_HD static uint64_t num_init(const Params &p) { return p.K; }
    MC_HD static void init(const Params &p, uint64_t k, WordRef out) { out.set(0, 0); out.set(1, p.h0 + k); }
    MC_HD static unsigned init_status(const Params &, CWordRef) { return ST_ENABLED; }
    MC_HD static uint64_t fp2(uint64_t x, uint64_t h) { return fp_nonzero(fmix64(x * 0x9e3779b97f4a7c15ull ^ fmix64(h + 1))); }
    MC_HD static uint64_t fp_of(const Params &, CWordRef s) { return fp2(s.get(0), s.get(1)); }
    MC_HD static void load(const Params &, CWordRef s, Local &l) { l.x = s.get(0); l.h = s.get(1); }
    MC_HD static int nslots(const Params &p, const Local &) { return 5 + p.B; }
    // the successor of (x, h) through `slot`; false: not enabled
    MC_HD static bool next(const Params &p, uint64_t x, uint64_t h, int slot, uint64_t &nx, uint64_t &nh) {
        nx = x;
        nh = h;
        if (slot == 0) { nx = x + 1; nh = 0; return h == (uint64_t)p.G; }
        if (slot == 1) { nh = h + 1; return h < (uint64_t)p.G; }
        if (slot == 2) { nh = h / 2; return p.on & ON_FOLD; }
        if (slot == 3) { nh = h ^ 1; return p.on & ON_SPIN; }
        if (slot < 4 + p.B) { nh = h * (uint64_t)p.B + (uint64_t)(slot - 4) + 1000; return true; }
        if (slot == 4 + p.B) { nx = x + 2; return p.on & ON_LEAK; }
        return false;
    }
    MC_HD static unsigned eval(const Params &p, const Local &l, CWordRef, int slot, uint64_t &fp) {
        uint64_t nx, nh;
        if (slot < 0 || !next(p, l.x, l.h, slot, nx, nh)) return 0;
        fp = fp2(nx, nh);
        return ST_ENABLED;
    }
    MC_HD static unsigned apply(const Params &p, CWordRef s, int slot, WordRef out) {
        uint64_t nx, nh;
        next(p, s.get(0), s.get(1), slot, nx, nh);
        out.set(0, nx);
        out.set(1, nh);
        return ST_ENABLED;
    }
};

// the host rule over SpecGap: out[b] for every behaviour of the batch
inline int gap_host(const SpecGap::Params &prm, uint64_t count, const uint64_t *first, const uint64_t *rows, const uint64_t *mask, unsigned flags,
                    mc_beh_verdict *out) {
    for (uint64_t b = 0; b < count; ++b)
        if (int rc = beh_check<SpecGap>(prm, rows + first[b] * 2, first[b + 1] - first[b], mask, flags, &out[b], nullptr)) return rc;
    return MC_OK;
}
}  // namespace mc
