// behaviour.h — "is this recorded execution a behaviour of the model?" (mc_engine_behaviours), the rule written once
// as MC_HD code: the device kernel (engine_behaviours.h, k_behaviours) decides with these functions, and beh_check below is the whole
// rule run on the host (mc_engine_behaviour_witness, tests/_behshim: what the kernel must reproduce field for field).
//
// A behaviour is a sequence of observations o_0 .. o_{T-1}, T >= 1, each a row in the lowering's layout (S::words words).  One mask m
// of the same width goes with a batch (none = everything is observed); a state s MATCHES o iff (s ^ o) & m == 0 on every word.
//   K_0 = the initial states init(k), k < num_init, that match o_0;
//   K_i = the distinct ROWS t that match o_i with t = apply(s, slot) for some s in K_{i-1} and a slot that eval(s, slot) enables;
//         under MC_BEH_F_STUTTER also every s in K_{i-1} that itself matches o_i (the stuttering step [Next]_vars allows).
// Unlogged steps (H = beh_hidden(flags) > 0): up to H model steps that leave every observed cell unchanged may lie between o_{i-1} and
// o_i.  K_i is then built from the closure C of K_{i-1}: C^0 = K_{i-1}; C^d = C^{d-1} plus the distinct rows, not in C^{d-1}, that
// match o_{i-1} and are a successor of a member that joined at depth d - 1; C = C^H (it stops when a depth adds nothing).  Every member
// of C is evaluated exactly once: each enabled slot counts in `generated`, the successor joins K_i if it matches o_i and — from a
// member of depth < H — C if it matches o_{i-1} and is new (it may join both).  No hidden step comes before o_0.  A C that would pass
// MC_BEH_MAX_CANDIDATES rows at depth d makes the behaviour AMBIGUOUS once the members of depth d - 1 are all evaluated (layers do not
// depend on order, so the counters stay a function of the behaviour).  With a full mask the fingerprint rules a successor out only
// when it is neither o_i's nor o_{i-1}'s.  peak covers |C| of every observation enumerated without ambiguity.  H = 0 is the rule above.
// How a successor counts (beh_step_kind): with ST_ASSERT, ST_SPECERR or ST_OVERFLOW it is no step (`errors`); with ST_OUT_OF_MODEL it
// IS a step — a CONSTRAINT bounds the search, not the system — and `outside` counts it where it matches; ST_INVARIANT is ignored.  A
// successor the lowering marks ST_SELFLOOP is its parent's row (it is not built with apply: the BFS never builds one either).
// Distinct is by row: under a VIEW two rows share a fingerprint.  The fingerprint eval gives is used to rule equality OUT (with a full
// mask a successor whose fingerprint is not o_i's is never built; two members of a set are compared word by word only where their
// fingerprints agree), never to assume it.  It is the stored successor's fingerprint only: beh_fp_known.
// Verdict: ACCEPTED (step = T) when K_{T-1} is non-empty; REJECTED at the first i whose K_i is empty; AMBIGUOUS at the first i whose
// K_i would hold more than MC_BEH_MAX_CANDIDATES rows — not decided, and nothing is ever dropped.  The counters cover every step up to
// and including the one that decides: generated = initial states built + enabled successors evaluated; peak = the largest set;
// candidates = the size of the last non-empty set.  All of it is a function of (behaviour, mask, flags) alone.
#pragma once
#include "mc_common.h"
#include "../../include/tlamc.h"

#include <algorithm>
#include <vector>

namespace mc {

enum : unsigned { BEH_RUNNING = 0 };   // a verdict word that is none of MC_BEH_ACCEPTED / REJECTED / AMBIGUOUS yet
enum : unsigned { BEH_NO_STEP = 0, BEH_STEP = 1, BEH_STEP_OUTSIDE = 2, BEH_ERROR = 3 };

// what an evaluated slot contributes: nothing (not enabled), an error, a step, a step that leaves the CONSTRAINTs
MC_HD unsigned beh_step_kind(unsigned st) {
    if (!(st & ST_ENABLED)) return BEH_NO_STEP;
    if (st & (ST_ASSERT | ST_SPECERR | ST_OVERFLOW)) return BEH_ERROR;
    return st & ST_OUT_OF_MODEL ? BEH_STEP_OUTSIDE : BEH_STEP;
}
// whether the fingerprint eval left is the successor row's (a lowering computes none for a successor it never stores)
MC_HD bool beh_fp_known(unsigned st) { return !(st & (ST_OUT_OF_MODEL | ST_SELFLOOP)); }

// (s ^ o) & m == 0 on every word; mask NULL = all ones
template <class Ref>
MC_HD bool beh_match(Ref s, const uint64_t *obs, const uint64_t *mask, int W) {
    uint64_t d = 0;
    for (int w = 0; w < W; ++w) d |= (s.get(w) ^ obs[w]) & (mask ? mask[w] : ~0ull);
    return d == 0;
}
template <class RefA, class RefB>
MC_HD bool beh_same_row(RefA a, RefB b, int W) {
    uint64_t d = 0;
    for (int w = 0; w < W; ++w) d |= a.get(w) ^ b.get(w);
    return d == 0;
}
MC_HD bool beh_mask_full(const uint64_t *mask, int W) {
    if (!mask) return true;
    for (int w = 0; w < W; ++w) if (mask[w] != ~0ull) return false;
    return true;
}

// the carry of a behaviour between two launches, one word: observations decided | size of the current set << 32 | verdict << 40
MC_HD uint64_t beh_carry(uint32_t step, unsigned n, unsigned verdict) { return (uint64_t)step | (uint64_t)(n & 0xffu) << 32 | (uint64_t)(verdict & 0xffu) << 40; }
MC_HD uint32_t beh_carry_step(uint64_t c) { return (uint32_t)c; }
MC_HD unsigned beh_carry_n(uint64_t c) { return (unsigned)(c >> 32 & 0xffu); }
MC_HD unsigned beh_carry_verdict(uint64_t c) { return (unsigned)(c >> 40 & 0xffu); }
// H of mc_beh_opts.flags: how many unlogged steps may lie between two observations
MC_HD unsigned beh_hidden(unsigned flags) { return flags >> 8 & 0xffu; }

// ------------------------------------------------------------------------------------------------ the rule on the host
// One member of a candidate set with the link that put it there first: the least slot, then the least parent row.  A closure member
// (depth > 0) keeps the link of its least depth, then least slot, then least parent.
struct BehMember {
    std::vector<uint64_t> row;
    uint64_t fp;
    int parent;     // index into the closure of the set before, whose first members are that set (-1: an initial state)
    int32_t slot;   // the slot taken (-1: an initial state, -2: a stuttering step)
    int depth = 0;  // hidden steps from a member of the set before (closure members only)
};
struct BehSets {
    std::vector<std::vector<BehMember>> sets;       // K_0 .. the last set built (filled when the caller asks for a witness)
    std::vector<std::vector<BehMember>> closures;   // closures[i]: the closure C that K_i was built from (closures[0] is empty)
};

// rows: T observations of W words each.  Fills *out; sets (optional): every candidate set built, for the witness.
template <class S>
int beh_check(const typename S::Params &prm, const uint64_t *rows, uint64_t T, const uint64_t *mask, unsigned flags, mc_beh_verdict *out, BehSets *sets) {
    const int W = S::words(prm);
    if (beh_mask_full(mask, W)) mask = nullptr;
    const bool full = mask == nullptr;
    const int H = (int)beh_hidden(flags);
    mc_beh_verdict v{};
    std::vector<BehMember> cur, nxt;   // cur: K_{i-1}, then its closure behind it
    std::vector<uint64_t> stage(W);
    bool ambiguous = false;
    // a matching row joins the next set unless the same ROW is there (then the lesser link stays: slots come in rising order per
    // parent, parents in set order)
    auto join = [&](const uint64_t *row, uint64_t fp, int parent, int32_t slot) {
        for (auto &m : nxt)
            if (m.fp == fp && beh_same_row(CWordRef{m.row.data(), 1}, CWordRef{row, 1}, W)) {
                if (slot >= 0 && (m.slot < 0 || slot < m.slot)) { m.slot = slot; m.parent = parent; }
                return;
            }
        if (nxt.size() + 1 > MC_BEH_MAX_CANDIDATES) { ambiguous = true; return; }
        nxt.push_back(BehMember{std::vector<uint64_t>(row, row + W), fp, parent, slot});
    };
    // a successor that still matches the observation before joins the closure at depth `depth` unless the same row is in it; false:
    // the closure would pass MC_BEH_MAX_CANDIDATES rows
    auto close = [&](const uint64_t *row, uint64_t fp, int parent, int32_t slot, int depth) {
        for (auto &m : cur)
            if (m.fp == fp && beh_same_row(CWordRef{row, 1}, CWordRef{m.row.data(), 1}, W)) {
                if (m.depth == depth && slot < m.slot) { m.slot = slot; m.parent = parent; }
                return true;
            }
        if (cur.size() + 1 > MC_BEH_MAX_CANDIDATES) return false;
        cur.push_back(BehMember{std::vector<uint64_t>(row, row + W), fp, parent, slot, depth});
        return true;
    };
    for (uint64_t i = 0; i < T && !v.verdict; ++i) {
        const uint64_t *obs = rows + i * W, *prev = i ? obs - W : obs;
        const uint64_t ofp = full ? S::fp_of(prm, CWordRef{obs, 1}) : 0;
        const uint64_t pfp = full && H ? S::fp_of(prm, CWordRef{prev, 1}) : ofp;
        nxt.clear();
        if (i == 0) {
            const uint64_t ni = S::num_init(prm);
            for (uint64_t k = 0; k < ni; ++k) {
                S::init(prm, k, WordRef{stage.data(), 1});
                v.generated++;
                if (!beh_match(CWordRef{stage.data(), 1}, obs, mask, W)) continue;
                if (S::init_status(prm, CWordRef{stage.data(), 1}) & ST_OUT_OF_MODEL) v.outside++;
                join(stage.data(), S::fp_of(prm, CWordRef{stage.data(), 1}), -1, -1);
            }
        } else {
            // every member of the closure is evaluated once, in the order it joined: depth by depth.  A closure that overflows at depth d
            // ends the observation once the members of depth d - 1 are through.
            int last_depth = H;
            for (size_t c = 0; c < cur.size() && cur[c].depth <= last_depth; ++c) {
                const std::vector<uint64_t> crow = cur[c].row;   // (cur grows)
                const uint64_t cfp = cur[c].fp;
                const int depth = cur[c].depth;
                const CWordRef s{crow.data(), 1};
                if ((flags & MC_BEH_F_STUTTER) && beh_match(s, obs, mask, W)) join(crow.data(), cfp, (int)c, -2);
                typename S::Local loc;
                S::load(prm, s, loc);
                const int ns = S::nslots(prm, loc);
                for (int slot = 0; slot < ns; ++slot) {
                    uint64_t f = 0;
                    const unsigned st = S::eval(prm, loc, s, slot, f);
                    const unsigned kind = beh_step_kind(st);
                    if (kind == BEH_NO_STEP) continue;
                    v.generated++;
                    if (kind == BEH_ERROR) { v.errors++; continue; }
                    const bool known = beh_fp_known(st);
                    if (full && known && f != ofp && f != pfp) continue;
                    if (st & ST_SELFLOOP) stage = crow;
                    else S::apply(prm, s, slot, WordRef{stage.data(), 1});
                    const bool to_next = beh_match(CWordRef{stage.data(), 1}, obs, mask, W);
                    const bool to_closure = depth < H && beh_match(CWordRef{stage.data(), 1}, prev, mask, W);
                    if (!to_next && !to_closure) continue;
                    const uint64_t fp = known ? f : S::fp_of(prm, CWordRef{stage.data(), 1});
                    if (to_next) {
                        if (kind == BEH_STEP_OUTSIDE) v.outside++;
                        join(stage.data(), fp, (int)c, slot);
                    }
                    if (to_closure && !close(stage.data(), fp, (int)c, slot, depth + 1)) { ambiguous = true; last_depth = depth; }
                }
            }
            if (!ambiguous && cur.size() > v.peak) v.peak = (uint32_t)cur.size();
        }
        if (sets && i) sets->closures.push_back(cur);
        if (ambiguous) { v.verdict = MC_BEH_AMBIGUOUS; v.step = (uint32_t)i; break; }
        if (nxt.empty()) { v.verdict = MC_BEH_REJECTED; v.step = (uint32_t)i; break; }
        v.candidates = (uint32_t)nxt.size();
        if (v.candidates > v.peak) v.peak = v.candidates;
        cur.swap(nxt);
        if (sets) {
            if (!i) sets->closures.emplace_back();
            sets->sets.push_back(cur);
        }
    }
    if (!v.verdict) { v.verdict = MC_BEH_ACCEPTED; v.step = (uint32_t)T; }
    *out = v;
    return MC_OK;
}

// One model path s_0 .. s_{n-1} through the sets beh_check built (n = v.step for a rejected or ambiguous behaviour, T for an
// accepted one): it ends in the least row of the last set and follows the links back.  slots[k]: the slot from s_{k-1} to s_k (-1
// for s_0, -2 for a stuttering step).
inline size_t beh_witness(const BehSets &bs, int W, uint64_t *states_out, int32_t *slots_out) {
    const size_t n = bs.sets.size();
    if (!n) return 0;
    const auto &last = bs.sets[n - 1];
    int at = 0;
    for (size_t c = 1; c < last.size(); ++c)
        if (std::lexicographical_compare(last[c].row.begin(), last[c].row.end(), last[at].row.begin(), last[at].row.end())) at = (int)c;
    for (size_t k = n; k-- > 0;) {
        const BehMember &m = bs.sets[k][at];
        std::copy(m.row.begin(), m.row.end(), states_out + k * W);
        slots_out[k] = m.slot;
        at = m.parent;
    }
    return n;
}

// The same path with the unlogged steps in it (mc_engine_behaviour_path): between the member of K_{k-1} and the member of K_k lie the
// closure members the links pass through.  obs[j]: the observation state j stands at (a hidden state repeats the one before it).
struct BehPath {
    std::vector<uint64_t> states;
    std::vector<int32_t> slots;
    std::vector<uint32_t> obs;
};
inline BehPath beh_path(const BehSets &bs, int W) {
    BehPath p;
    const size_t n = bs.sets.size();
    if (!n) return p;
    const auto &last = bs.sets[n - 1];
    int at = 0;
    for (size_t c = 1; c < last.size(); ++c)
        if (std::lexicographical_compare(last[c].row.begin(), last[c].row.end(), last[at].row.begin(), last[at].row.end())) at = (int)c;
    std::vector<const BehMember *> back;   // the path from its end
    std::vector<uint32_t> back_obs;
    for (size_t k = n; k-- > 0;) {
        const BehMember *m = &bs.sets[k][at];
        back.push_back(m);
        back_obs.push_back((uint32_t)k);
        at = m->parent;
        if (!k) break;
        while (bs.closures[k][at].depth > 0) {   // (depth falls by one per link: at most H of them)
            m = &bs.closures[k][at];
            back.push_back(m);
            back_obs.push_back((uint32_t)k - 1);
            at = m->parent;
        }
    }
    for (size_t j = back.size(); j-- > 0;) {
        p.states.insert(p.states.end(), back[j]->row.begin(), back[j]->row.begin() + W);
        p.slots.push_back(back[j]->slot);
        p.obs.push_back(back_obs[j]);
    }
    return p;
}

}  // namespace mc
