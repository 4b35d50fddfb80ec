// engine_sim.h — the DEVICE half of simulation mode (mc_engine_simulate, TLC's `-simulate`): k_simulate, one lane per random walk.
// Included by engine.hip only (inside namespace mc, after engine_kernels.h: arena_ref / arena_cref, the wave reductions).
//
// A round of walks w0 .. w0+n-1 keeps its current states in two walk buffers with the arena's strided-64 layout (lane l of a
// wavefront owns column l of a 64-state block, so every row access of a wavefront is coalesced); state number i of a walk lives in
// buffer i & 1, so a step reads one buffer and writes the other.  Each launch advances every walk of the round by at most `iters`
// events of sim_walk.h's sim_step (a bounded amount of work: the host stops, reports and checks between launches); what a walk needs
// across launches is one word (states reached | end reason << 24).  The slot loop runs to the wavefront's largest nslots, as in
// k_expand.  Counters: one atomic of each kind per wavefront and launch; the violation: an atomicMin on the walk's key.
#ifndef TLAMC_ENGINE_SIM_H
#define TLAMC_ENGINE_SIM_H

#include "sim_walk.h"

namespace mc {

struct SimCounters {
    unsigned long long generated;   // enabled successors evaluated (+ initial states)
    unsigned long long steps;       // states reached
    unsigned long long walks;       // walks ended
    unsigned long long viol;        // min violation key (sim_key), ~0 = none
    unsigned int max_depth;         // longest ended walk (states)
    unsigned int error;             // DEV_EOVERFLOW
};

struct SimArgs {
    uint64_t seed, w0, n, ncols;     // lanes 0 .. ncols-1 (a multiple of 64); lane l < n runs walk w0 + l
    uint64_t *buf0, *buf1;           // the two walk buffers (strided-64 rows of S::words each)
    uint32_t *wst;                   // per lane: states reached | end << 24
    uint32_t depth, iters, deadlock;
    SimCounters *ctr;
    // record mode: walks rec_first .. rec_first + rec_count - 1 leave their slot sequence (rec_slots[k * depth + s]: the slot from
    // state s to state s + 1), their length and their end reason; rec_rows (one walk, rec_count = 1): its states as plain rows, plus
    // the violating successor of an invariant broken by a step
    uint64_t rec_first, rec_count;
    int32_t *rec_slots;
    uint32_t *rec_len, *rec_end;
    uint64_t *rec_rows;
};

template <class S>
__global__ void __launch_bounds__(256)
k_simulate(typename S::Params prm, SimArgs a) {
    const uint64_t col = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= a.ncols) return;  // ncols is a multiple of 64: whole wavefronts leave together
    const bool active = col < a.n;
    const int W = S::words(prm);
    const uint32_t ws = active ? a.wst[col] : ((uint32_t)SIM_END_DEPTH << 24);
    SimWalk wk;
    sim_begin(wk, a.seed, a.w0 + col, ws & 0xffffffu, ws >> 24);
    const uint32_t t0 = wk.t;
    const bool was_running = wk.end == SIM_RUNNING;
    const uint64_t ri = wk.walk - a.rec_first;
    const bool rec = active && a.rec_slots && ri < a.rec_count;
    for (uint32_t it = 0; it < a.iters; ++it) {
        if (!wave_or_u32(wk.end == SIM_RUNNING ? 1u : 0u)) break;   // (uniform: every lane of the wavefront is here)
        const uint32_t t = wk.t, end0 = wk.end;
        const CWordRef cur = arena_cref((t + 1) & 1 ? a.buf1 : a.buf0, col, W);
        const WordRef nxt = arena_ref(t & 1 ? a.buf1 : a.buf0, col, W);
        sim_step<S>(prm, wk, a.depth, a.deadlock, cur, nxt, [](int ns) { return (int)wave_max_u32((unsigned)ns); });
        if (rec) {
            if (wk.slot >= 0) a.rec_slots[ri * a.depth + (wk.t - 2)] = wk.slot;
            if (a.rec_rows) {
                if (wk.t > t)
                    for (int w = 0; w < W; ++w) a.rec_rows[(uint64_t)(wk.t - 1) * W + w] = nxt.get(w);
                if (end0 == SIM_RUNNING && wk.end == SIM_END_VIOLATION && sim_key_kind(wk.viol) == SIM_VK_INVARIANT &&
                    sim_key_slot(wk.viol) < SIM_SLOT_PARENT)  // the successor that breaks the invariant is a row of the trace too
                    S::apply(prm, cur, (int)sim_key_slot(wk.viol), WordRef{a.rec_rows + (uint64_t)t * W, 1});
            }
            if (end0 == SIM_RUNNING && wk.end != SIM_RUNNING) { a.rec_len[ri] = wk.t; a.rec_end[ri] = wk.end; }
        }
    }
    const bool ended = active && was_running && wk.end != SIM_RUNNING;
    if (active) a.wst[col] = wk.t | (wk.end << 24);
    const unsigned gsum = wave_sum_u32(active ? wk.gen : 0u);
    const unsigned ssum = wave_sum_u32(active ? wk.t - t0 : 0u);
    const unsigned esum = wave_sum_u32(ended ? 1u : 0u);
    const unsigned dmax = wave_max_u32(ended ? wk.t : 0u);
    const unsigned long long vmin = wave_min_u64(active ? wk.viol : ~0ull);
    const unsigned eor = wave_or_u32(active && wk.end == SIM_END_OVERFLOW ? (unsigned)DEV_EOVERFLOW : 0u);
    if ((threadIdx.x & 63) == 0) {
        if (gsum) atomicAdd(&a.ctr->generated, (unsigned long long)gsum);
        if (ssum) atomicAdd(&a.ctr->steps, (unsigned long long)ssum);
        if (esum) atomicAdd(&a.ctr->walks, (unsigned long long)esum);
        if (dmax) atomicMax(&a.ctr->max_depth, dmax);
        if (vmin != ~0ull) atomicMin(&a.ctr->viol, vmin);
        if (eor) atomicOr(&a.ctr->error, eor);
    }
}

}  // namespace mc

#endif  // TLAMC_ENGINE_SIM_H
