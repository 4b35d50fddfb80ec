// sim_walk.h — one random walk of TLC's simulation mode (`tlc -simulate`), written once as MC_HD code: the device kernel
// (engine_sim.h, k_simulate) and the host (tests/_simshim, the walk the kernel must reproduce) run exactly this.
//
// A walk w of a run (seed, num, depth) is a function of (seed, w, depth) alone:
//   * its initial state is init(k), k = H(seed, w) mod num_init;
//   * at every step each slot 0 .. nslots-1 of the current state is evaluated with S::eval, as the BFS evaluates it, and every
//     enabled successor is checked as the BFS checks it (Assert, invariants, evaluation errors, slot-array overflow);
//   * the next state is the enabled, in-model, non-stuttering successor whose slot has the least H(seed, w, step, slot) (the lower
//     slot on a tie): no per-slot masks, uniform over the candidates; one pass, and one more for every stuttering successor that only
//     shows when it is built (a row equal to its parent's) and is then passed over;
//   * every state reached is checked with init_status (the initial state) and the stored-state invariants (all of them);
//   * the walk ends at `depth` states, at its first violation, at a deadlock, or when no in-model, non-stuttering successor is left.
// So every state a walk reaches is one the BFS stores (tests/test_simulate_host.py).  Compiles without HIP (spec_*.h do too).
#pragma once
#include "mc_common.h"

namespace mc {

// why a walk ended (mc_sim_result / the recorded walks of tlamc.h: MC_SIM_END_*)
enum : unsigned {
    SIM_RUNNING = 0,
    SIM_END_DEPTH = 1,         // it reached `depth` states
    SIM_END_VIOLATION = 2,     // invariant, Assert, evaluation error, or a deadlock with deadlock checking on
    SIM_END_DEADLOCK = 3,      // no enabled successor, deadlock checking off
    SIM_END_OUT_OF_MODEL = 4,  // every enabled successor is outside the CONSTRAINTs (or the initial state is)
    SIM_END_STUTTER = 5,       // only stuttering successors are left
    SIM_END_OVERFLOW = 6       // a fixed-capacity slot array of the packed state is full (the run fails with MC_EOVERFLOW)
};
// violation kinds and the slot codes of a key (the same values as the BFS's VK_* / SLOT_* of engine_kernels.h)
enum : unsigned { SIM_VK_INVARIANT = 1, SIM_VK_ASSERT = 2, SIM_VK_DEADLOCK = 3, SIM_VK_SPECERR = 4 };
static constexpr unsigned SIM_SLOT_NONE = 0xffffu, SIM_SLOT_INIT = 0xfffeu, SIM_SLOT_PARENT = 0xfffdu;

// violation key: min over a round = the lowest walk index, then the lowest slot.  Walk indices below 2^40.
MC_HD unsigned long long sim_key(uint64_t walk, unsigned slot, unsigned kind, unsigned inv) {
    return ((unsigned long long)walk << 24) | ((unsigned long long)(slot & 0xffffu) << 8) | ((inv & 31u) << 3) | (kind & 7u);
}
MC_HD uint64_t sim_key_walk(unsigned long long k) { return (uint64_t)(k >> 24); }
MC_HD unsigned sim_key_slot(unsigned long long k) { return (unsigned)(k >> 8 & 0xffffu); }
MC_HD unsigned sim_key_kind(unsigned long long k) { return (unsigned)(k & 7u); }
MC_HD unsigned sim_key_inv(unsigned long long k) { return (unsigned)(k >> 3 & 31u); }

// H: counter-based, fmix64 over (seed, walk), then (step), then (slot)
MC_HD uint64_t sim_walk_hash(uint64_t seed, uint64_t walk) {
    return fmix64(fmix64(seed ^ 0x243f6a8885a308d3ull) ^ (walk * 0x9e3779b97f4a7c15ull + 0x13198a2e03707344ull));
}
MC_HD uint64_t sim_step_hash(uint64_t walk_hash, uint32_t step) { return fmix64(walk_hash ^ ((uint64_t)step * 0xc2b2ae3d27d4eb4full)); }
MC_HD uint64_t sim_slot_hash(uint64_t step_hash, int slot) { return fmix64(step_hash + ((uint64_t)slot + 1u) * 0x165667b19e3779f9ull); }

// invariants of a reached state: S::parent_status_step where the lowering has it (its verdict from what the last step can have changed),
// else S::parent_status — as the BFS's stored_state_status (engine_kernels.h), which is device-only
template <class S, class = void>
struct SimStepStatus { static constexpr bool value = false; };
template <class S>
struct SimStepStatus<S, decltype((void)S::STEP_STATUS)> { static constexpr bool value = true; };
template <class S>
MC_HD unsigned sim_state_status(const typename S::Params &prm, const typename S::Local &loc, CWordRef s) {
    if constexpr (SimStepStatus<S>::value) return S::parent_status_step(prm, loc, s);
    else return S::parent_status(prm, loc, s);
}

// One walk's registers between two calls of sim_step.
struct SimWalk {
    uint64_t walk;              // index w
    uint64_t hash;              // H(seed, w)
    uint32_t t;                 // states reached so far (the current state is state t - 1)
    uint32_t end;               // SIM_RUNNING or SIM_END_*
    unsigned long long viol;    // ~0 or the walk's violation key
    int32_t slot;               // slot taken by the last call (-1: none, or the call started / ended the walk)
    uint32_t gen;               // enabled successors (and the initial state) evaluated, summed over calls
};
MC_HD void sim_begin(SimWalk &wk, uint64_t seed, uint64_t walk, uint32_t t, uint32_t end) {
    wk.walk = walk;
    wk.hash = sim_walk_hash(seed, walk);
    wk.t = t;
    wk.end = end;
    wk.viol = ~0ull;
    wk.slot = -1;
    wk.gen = 0;
}

// One event of a walk: a walk with t = 0 builds its initial state into `nxt`; otherwise the current state `cur` is checked, expanded,
// and its chosen successor written to `nxt` (t + 1), or the walk ends.  `bound(ns)` gives the trip count of the slot loop and says
// whether another pass is due: ns on the host, the wavefront's maximum on the device (every lane of a wavefront calls it, at the same
// points: its lanes that take no step pass 0).  flags: MC_F_DEADLOCK.
template <class S, class Bound>
MC_HD void sim_step(const typename S::Params &prm, SimWalk &wk, uint32_t depth, unsigned deadlock, CWordRef cur, WordRef nxt, Bound &&bound) {
    wk.slot = -1;
    typename S::Local loc;
    int ns = 0;
    bool expand = false;
    if (wk.end == SIM_RUNNING && wk.t == 0) {
        const uint64_t ni = S::num_init(prm);
        S::init(prm, ni ? wk.hash % ni : 0, nxt);
        wk.gen++;
        const unsigned st = S::init_status(prm, CWordRef{nxt.p, nxt.stride});
        if (st & ST_INVARIANT) {
            wk.viol = sim_key(wk.walk, SIM_SLOT_INIT, SIM_VK_INVARIANT, st >> 8);
            wk.end = SIM_END_VIOLATION;
            wk.t = 1;
        } else if (st & ST_OUT_OF_MODEL) {
            wk.end = SIM_END_OUT_OF_MODEL;   // reached nothing: the BFS does not store it either
        } else {
            wk.t = 1;
        }
    } else if (wk.end == SIM_RUNNING) {
        S::load(prm, cur, loc);
        const unsigned ps = sim_state_status<S>(prm, loc, cur);
        if (ps & ST_INVARIANT) {
            wk.viol = sim_key(wk.walk, SIM_SLOT_PARENT, SIM_VK_INVARIANT, ps >> 8);
            wk.end = SIM_END_VIOLATION;
        } else if (wk.t >= depth) {
            wk.end = SIM_END_DEPTH;
        } else {
            expand = true;
            ns = S::nslots(prm, loc);
        }
    }
    const uint64_t sh = sim_step_hash(wk.hash, wk.t);
    const int W = S::words(prm);
    unsigned gen = 0, stutter = 0, overflow = 0;
    unsigned long long viol = ~0ull;
    // A pass evaluates every slot and picks the candidate with the least (hash, slot) above `floor`.  A lowering marks the stuttering
    // successors it knows of (ST_SELFLOOP); one it does not mark (the terminating disjunct of a PlusCal translation, a label whose body
    // changes nothing) shows when it is built: the row equals its parent.  It is then passed over and the next candidate in hash order
    // taken by one more pass, so the choice stays uniform over the non-stuttering candidates.  Every lane of a wavefront makes the
    // same number of passes (bound() is a wavefront operation on the device).
    uint64_t floor_h = 0;
    int floor_slot = -1;
    bool first = true, again = expand;
    while (bound(again ? 1 : 0)) {
        const int wns = bound(again ? ns : 0);
        uint64_t best = ~0ull;
        int pick = -1;
        for (int slot = 0; slot < wns; ++slot) {
            if (again && slot < ns) {
                uint64_t f = 0;
                const unsigned st = S::eval(prm, loc, cur, slot, f);
                if (st & ST_ENABLED) {
                    if (first) ++gen;
                    if (st & ST_OVERFLOW) overflow = 1;
                    else if (st & ST_ASSERT) viol = viol < sim_key(wk.walk, slot, SIM_VK_ASSERT, 0) ? viol : sim_key(wk.walk, slot, SIM_VK_ASSERT, 0);
                    else if (st & ST_SPECERR) viol = viol < sim_key(wk.walk, slot, SIM_VK_SPECERR, 0) ? viol : sim_key(wk.walk, slot, SIM_VK_SPECERR, 0);
                    else {
                        if (st & ST_INVARIANT) {
                            const unsigned long long k = sim_key(wk.walk, slot, SIM_VK_INVARIANT, st >> 8);
                            viol = viol < k ? viol : k;
                        }
                        if (st & ST_SELFLOOP) stutter = 1;
                        else if (!(st & ST_OUT_OF_MODEL)) {
                            const uint64_t h = sim_slot_hash(sh, slot);
                            const bool above = floor_slot < 0 || h > floor_h || (h == floor_h && slot > floor_slot);
                            if (above && (h < best || pick < 0)) { best = h; pick = slot; }
                        }
                    }
                }
            }
        }
        if (!again) continue;
        again = false;
        if (first) {
            first = false;
            wk.gen += gen;
            if (overflow) { wk.end = SIM_END_OVERFLOW; continue; }
            if (viol != ~0ull) { wk.viol = viol; wk.end = SIM_END_VIOLATION; continue; }
            if (gen == 0) {
                if (deadlock) { wk.viol = sim_key(wk.walk, SIM_SLOT_NONE, SIM_VK_DEADLOCK, 0); wk.end = SIM_END_VIOLATION; }
                else wk.end = SIM_END_DEADLOCK;
                continue;
            }
        }
        if (pick < 0) { wk.end = stutter ? SIM_END_STUTTER : SIM_END_OUT_OF_MODEL; continue; }
        S::apply(prm, cur, pick, nxt);
        bool same = true;
        for (int w = 0; w < W; ++w) same = same && nxt.get(w) == cur.get(w);
        if (same) { stutter = 1; floor_h = best; floor_slot = pick; again = true; continue; }
        wk.slot = pick;
        wk.t++;
    }
}

}  // namespace mc
