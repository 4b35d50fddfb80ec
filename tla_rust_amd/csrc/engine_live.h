// engine_live.h — the DEVICE half of the strongly-connected-components pass (mc_engine_scc) and of the fairness check built on it
// (mc_engine_liveness), and the library's two device scans.  Included by state_graph.hip only: one copy in the library, whatever the
// lowering of the engine that asks.  Everything here is a consumer of the CSR arrays of mc_engine_graph (offsets / dst / proc) and of
// nothing else; k_live_proc<S>, which walks the arena once more to say which process instance takes each edge, is beside the other
// spec-walking kernels in engine_graph.h.  The rule itself is liveness.h's, MC_HD code the host runs too.
//
//   transpose   k_live_indegree (atomics) -> hipcub exclusive scan in 64 bits -> k_live_tfill.  Edges that end where they start are left
//               out: no consumer wants them.  A row of the transpose is in no particular order (the fill's atomics decide); every reader
//               either looks at the whole row or takes its least entry.
//   SCC         trim, then colouring, repeated until no state is live (scc[v] == SCC_LIVE):
//                 k_scc_trim     a live state with no live in-edge or no live out-edge is its own component
//                 k_scc_colour   colour[v] = max(colour[v], colour[u]) over the live in-edges u -> v, to a fixed point: the largest arena
//                                index that reaches v.  The states with colour[v] == v are roots (k_scc_roots).
//                 k_scc_back     a live state with an out-edge to a state already given to ITS colour's root joins that root: backward
//                                reachability from the root inside its colour class = the root's component
//               then k_scc_least / k_scc_renumber: scc[v] = the LEAST arena index of v's component (roots are the largest), so the
//               numbering is a function of the graph alone; k_scc_sizes counts the members.
//               One lane per state over its CSR row; rows of one wavefront's lanes have any lengths (every loop is the lane's own, no
//               wavefront operation inside).  A sweep that changed something sets a per-workgroup bit in LDS, and one lane of the
//               workgroup raises the device flag; the host reads the flag once per SCC_BATCH sweeps.  Sweeps update in place: a lane may
//               see a value another lane wrote in the same sweep — every update is monotone (live -> assigned, colours only grow), so that
//               only makes the fixed point come sooner.
//   fairness    k_live_reduce    per state the en / taken masks and the Done flag (live_state), OR-ed into the component's entry at
//                                scc[v]: plain stores for one-state components, else one atomic per set of lanes that agree on it
//               k_live_verdict   per component root the rule (live_violates); the number of fair non-Done components and the least root
//   properties  (mc_engine_liveness_check) the same over the subgraph induced by a mask M of predicate bits:
//               k_scc_mask       before the first trim: a state outside M is a component of its own, and live to nobody
//               k_live_reduce<true> / k_live_verdict<true>   only states of M are merged and judged, "holds a T state" in the Done
//                                flag's place; en comes from the full row, taken from edges whose two ends share the component
//               k_live_reach     dist[v], to a fixed point: 0 in a violating component, else 1 + the least dist of a successor in M
//               k_live_witness   the states of M, the S states with a dist, and the least of those
//   strong      (mc_engine_liveness_strong / mc_engine_liveness_check_strong) the refinement, one round per loop:
//               k_live_open_init every state of M open, refined ids = own index
//               k_scc_open       rounds >= 2, before the first trim: a state that is not open is a component of its own
//               k_live_reduce    as above, over the round's components (a closed state merges into its own entry: nobody reads it)
//               k_live_enabled   en of the open states, OR-ed per component into enabled[]
//               k_live_classify  per root of an open component: the final violating components, counted, and the least root
//               k_live_refine    per open state: closed / still open / final; a final state takes its component's id and size into the
//                                refined arrays and dist 0; states closed and "some state is still open", one atomic per wavefront
//               then k_live_reach / k_live_witness as above
//   units       (mc_engine_liveness_units / mc_engine_liveness_check_units) the refinement with the edges' UNITS in
//               proc[]'s place and masks of fairness CONJUNCTS: k_live_reduce_units / k_live_enabled_units / k_live_refine_units stage
//               of_unit[] in LDS and run the bodies of their process-level twins, instantiated for the table; the twins stay the code
//               they were.  Everything that reads masks alone (k_live_classify, the reach pass, the witness) serves both.
//
// Memory, beside the graph's 8 bytes per state and 6 per edge: 16 bytes per state (transpose offsets 8, scc 4, colour / size 4) and 4 per
// edge (transpose) for mc_engine_scc, 4 more per state while the transpose is built; mc_engine_liveness adds 1 byte per edge (proc) and 20
// per state (taken 8, disabled 8, Done 4).  A strong check adds 25 per state: enabled 8, open / closed / final 1, the refined ids and
// sizes 8, the working ids and sizes of rounds >= 2 another 8.  A check by units adds 1 byte per edge (unit) and the table's 1 KiB.
#ifndef TLAMC_ENGINE_LIVE_H
#define TLAMC_ENGINE_LIVE_H

#include <hipcub/hipcub.hpp>

#include "liveness.h"
#include "state_graph.h"

namespace mc {

constexpr uint32_t SCC_LIVE = 0xffffffffu;   // scc[v] of a state no component has been found for yet
constexpr int SCC_BATCH = 8;                 // sweeps launched between two reads of the "changed" flag

struct LiveCounters {
    unsigned long long components, nontrivial, fair_components;
    unsigned largest, first_root;   // first_root: the least root among the fair non-Done components, ~0u = none
};

// (engine_kernels.h has the same reduction for the search kernels; that file is no part of this unit)
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) { unsigned t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

// the workgroup's "changed" bit: LDS, then one store to the device flag
__device__ __forceinline__ void live_raise(bool changed, unsigned *flag) {
    __shared__ unsigned wg_changed;
    if (threadIdx.x == 0) wg_changed = 0;
    __syncthreads();
    if (changed) wg_changed = 1;   // (every writer writes 1)
    __syncthreads();
    if (threadIdx.x == 0 && wg_changed) *flag = 1;
}

// ---- transpose
static __global__ void __launch_bounds__(256)
k_live_indegree(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, uint32_t *indeg) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    for (uint64_t k = offsets[v], end = offsets[v + 1]; k < end; ++k) {
        const uint32_t d = dst[k];
        if (d != (uint32_t)v && d < n) atomicAdd(&indeg[d], 1u);
    }
}
static __global__ void __launch_bounds__(256)
k_live_tfill(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, const uint64_t *__restrict__ toff,
             uint32_t *cursor, uint32_t *__restrict__ tsrc) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    for (uint64_t k = offsets[v], end = offsets[v + 1]; k < end; ++k) {
        const uint32_t d = dst[k];
        if (d == (uint32_t)v || d >= n) continue;
        const uint64_t at = toff[d] + atomicAdd(&cursor[d], 1u);
        if (at < toff[d + 1]) tsrc[at] = (uint32_t)v;   // (k_live_indegree counted this edge: the bound holds, and is checked all the same)
    }
}

// ---- SCC
static __global__ void __launch_bounds__(256)
k_scc_trim(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, const uint64_t *__restrict__ toff,
           const uint32_t *__restrict__ tsrc, uint32_t *scc, unsigned *flag) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool changed = false;
    if (v < n && scc[v] == SCC_LIVE) {
        bool out = false, in = false;
        for (uint64_t k = offsets[v], end = offsets[v + 1]; k < end && !out; ++k) {
            const uint32_t d = dst[k];
            out = d != (uint32_t)v && d < n && scc[d] == SCC_LIVE;
        }
        for (uint64_t k = toff[v], end = toff[v + 1]; out && k < end && !in; ++k) in = scc[tsrc[k]] == SCC_LIVE;   // (the transpose holds no self loop)
        if (!out || !in) { scc[v] = (uint32_t)v; changed = true; }
    }
    live_raise(changed, flag);
}
// the masked build: scc[] is all SCC_LIVE when this runs
static __global__ void __launch_bounds__(256)
k_scc_mask(uint64_t n, const uint32_t *__restrict__ pred, LiveCheck ck, uint32_t *__restrict__ scc) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n && live_own_component(ck, pred[v])) scc[v] = (uint32_t)v;
}
static __global__ void __launch_bounds__(256)
k_scc_colour_init(uint64_t n, const uint32_t *__restrict__ scc, uint32_t *__restrict__ colour, unsigned *flag) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = v < n && scc[v] == SCC_LIVE;
    if (v < n) colour[v] = (uint32_t)v;
    live_raise(live, flag);   // (here the flag says: some state is still live)
}
static __global__ void __launch_bounds__(256)
k_scc_colour(uint64_t n, const uint64_t *__restrict__ toff, const uint32_t *__restrict__ tsrc, const uint32_t *__restrict__ scc,
             uint32_t *colour, unsigned *flag) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool changed = false;
    if (v < n && scc[v] == SCC_LIVE) {
        const uint32_t mine = colour[v];
        uint32_t c = mine;
        for (uint64_t k = toff[v], end = toff[v + 1]; k < end; ++k) {
            const uint32_t u = tsrc[k];
            if (scc[u] != SCC_LIVE) continue;
            const uint32_t cu = colour[u];
            c = cu > c ? cu : c;
        }
        if (c > mine) { colour[v] = c; changed = true; }
    }
    live_raise(changed, flag);
}
static __global__ void __launch_bounds__(256)
k_scc_roots(uint64_t n, uint32_t *__restrict__ scc, const uint32_t *__restrict__ colour) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n && scc[v] == SCC_LIVE && colour[v] == (uint32_t)v) scc[v] = (uint32_t)v;
}
// (a root is live when its colour is computed, so no state was given to it before this round: scc[d] == colour[v] means "d reaches the
// root of v's colour class and is of that class")
static __global__ void __launch_bounds__(256)
k_scc_back(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, uint32_t *scc,
           const uint32_t *__restrict__ colour, unsigned *flag) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool changed = false;
    if (v < n && scc[v] == SCC_LIVE) {
        const uint32_t c = colour[v];
        for (uint64_t k = offsets[v], end = offsets[v + 1]; k < end; ++k) {
            const uint32_t d = dst[k];
            if (d != (uint32_t)v && d < n && scc[d] == c && colour[d] == c) { scc[v] = c; changed = true; break; }
        }
    }
    live_raise(changed, flag);
}
static __global__ void __launch_bounds__(256)
k_scc_least(uint64_t n, const uint32_t *__restrict__ scc, uint32_t *least) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const uint32_t r = scc[v];
    if (r < n && r != (uint32_t)v) atomicMin(&least[r], (uint32_t)v);   // (a root is its component's LARGEST index: only smaller ones matter)
}
static __global__ void __launch_bounds__(256)
k_scc_renumber(uint64_t n, uint32_t *__restrict__ scc, const uint32_t *__restrict__ least) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const uint32_t r = scc[v];
    if (r < n) { const uint32_t l = least[r]; scc[v] = l < r ? l : r; }
}
static __global__ void __launch_bounds__(256)
k_scc_sizes(uint64_t n, const uint32_t *__restrict__ scc, uint32_t *size) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const uint32_t r = scc[v];
    if (r < n) atomicAdd(&size[r], 1u);
}
static __global__ void __launch_bounds__(256)
k_scc_stats(uint64_t n, const uint32_t *__restrict__ scc, const uint32_t *__restrict__ size, LiveCounters *lc) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = v < n && scc[v] == (uint32_t)v;
    const unsigned sz = root ? size[v] : 0u;
    const unsigned roots = (unsigned)__popcll(__ballot(root)), big = (unsigned)__popcll(__ballot(sz > 1)), wmax = wave_max_u32(sz);
    if ((threadIdx.x & 63) == 0 && roots) {
        atomicAdd(&lc->components, (unsigned long long)roots);
        if (big) atomicAdd(&lc->nontrivial, (unsigned long long)big);
        atomicMax(&lc->largest, wmax);
    }
}

// ---- fairness
__device__ __forceinline__ unsigned long long wave_or_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// The table-driven forms: of_unit[] (LIVE_UNIT_TAB entries in device memory) is staged in LDS at block start and
// indexed per edge from there — a per-lane index into a by-value kernel argument would end up in scratch.  Every thread of the block
// gets here (no kernel below returns early).
__device__ __forceinline__ void live_stage_units(const uint64_t *__restrict__ of_unit, uint64_t *tab) {
    if (threadIdx.x < (unsigned)LIVE_UNIT_TAB) tab[threadIdx.x] = of_unit[threadIdx.x];
    __syncthreads();
}

// MASKED: scc / size are those of G[M]; only the states of M are merged, and `done` says "the component holds a T state"
// UNITS: proc[] holds units and of_unit (LDS) maps them to conjuncts; else of_unit is not read and the code is the process-level one
template <bool MASKED, bool UNITS>
__device__ __forceinline__ void
live_reduce_body(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, const int8_t *__restrict__ proc,
                 const uint32_t *__restrict__ scc, const uint32_t *__restrict__ size, uint64_t all, unsigned long long *taken,
                 unsigned long long *disabled, unsigned *done, const uint32_t *__restrict__ pred, LiveCheck ck, const uint64_t *of_unit) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = v < n && (!MASKED || live_in_mask(ck, pred[v]));
    uint64_t en = 0, tk = 0;
    bool dn = false;
    uint32_t comp = 0;
    if (active) {
        const uint64_t o = offsets[v];
        if constexpr (MASKED && UNITS) {
            live_state_masked_units((uint32_t)v, dst + o, proc + o, offsets[v + 1] - o, scc, of_unit, [&](uint32_t d) { return d < n && live_in_mask(ck, pred[d]); }, &en, &tk);
            dn = live_in_target(ck, pred[v]);
        } else if constexpr (UNITS) {
            live_state_units((uint32_t)v, dst + o, proc + o, offsets[v + 1] - o, scc, of_unit, &en, &tk, &dn);
        } else if constexpr (MASKED) {
            live_state_masked((uint32_t)v, dst + o, proc + o, offsets[v + 1] - o, scc, [&](uint32_t d) { return d < n && live_in_mask(ck, pred[d]); }, &en, &tk);
            dn = live_in_target(ck, pred[v]);
        } else {
            live_state((uint32_t)v, dst + o, proc + o, offsets[v + 1] - o, scc, &en, &tk, &dn);
        }
        comp = scc[v];
    }
    const uint64_t dis = active ? live_disabled(all, en) : 0;
    // a one-state component has one writer; the entries were cleared before the launch
    const bool alone = active && size[comp] == 1;
    if (alone) { taken[comp] = tk; disabled[comp] = dis; done[comp] = dn ? 1u : 0u; }
    // the others: one atomic per set of lanes that agree on the component (the loop's condition is the same in every lane)
    unsigned long long rest = __ballot(active && !alone);
    const unsigned lane = threadIdx.x & 63;
    while (rest) {
        const int lead = __ffsll((long long)rest) - 1;
        const uint32_t c0 = (uint32_t)__shfl((int)comp, lead);
        const bool same = active && !alone && comp == c0;
        const unsigned long long t = wave_or_u64(same ? tk : 0ull), d = wave_or_u64(same ? dis : 0ull);
        const unsigned long long dd = __ballot(same && dn);
        if ((int)lane == lead) {
            if (t) atomicOr(&taken[c0], t);
            if (d) atomicOr(&disabled[c0], d);
            if (dd) atomicOr(&done[c0], 1u);
        }
        rest &= ~__ballot(same);
    }
}
template <bool MASKED>
static __global__ void __launch_bounds__(256)
k_live_reduce(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, const int8_t *__restrict__ proc,
              const uint32_t *__restrict__ scc, const uint32_t *__restrict__ size, uint64_t all, unsigned long long *taken,
              unsigned long long *disabled, unsigned *done, const uint32_t *__restrict__ pred, LiveCheck ck) {
    live_reduce_body<MASKED, false>(n, offsets, dst, proc, scc, size, all, taken, disabled, done, pred, ck, nullptr);
}
template <bool MASKED>
static __global__ void __launch_bounds__(256)
k_live_reduce_units(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, const int8_t *__restrict__ unit,
                    const uint32_t *__restrict__ scc, const uint32_t *__restrict__ size, uint64_t all, unsigned long long *taken,
                    unsigned long long *disabled, unsigned *done, const uint32_t *__restrict__ pred, LiveCheck ck,
                    const uint64_t *__restrict__ of_unit) {
    __shared__ uint64_t tab[LIVE_UNIT_TAB];
    live_stage_units(of_unit, tab);
    live_reduce_body<MASKED, true>(n, offsets, dst, unit, scc, size, all, taken, disabled, done, pred, ck, tab);
}

// MASKED: only the components of states in M are judged, by live_violates_masked; dist[v] = 0 at a violating root, LIVE_FAR elsewhere
template <bool MASKED>
static __global__ void __launch_bounds__(256)
k_live_verdict(uint64_t n, const uint32_t *__restrict__ scc, const uint32_t *__restrict__ size, const unsigned long long *__restrict__ taken,
               const unsigned long long *__restrict__ disabled, const unsigned *__restrict__ done, uint64_t all, uint64_t fair, LiveCounters *lc,
               const uint32_t *__restrict__ pred, LiveCheck ck, uint32_t *__restrict__ dist) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = v < n && scc[v] == (uint32_t)v;
    const bool bad = root && (MASKED ? live_in_mask(ck, pred[v]) && live_violates_masked(all, fair, taken[v], disabled[v], done[v] != 0, size[v])
                                     : live_violates(all, fair, taken[v], disabled[v], done[v] != 0, size[v]));
    if (MASKED && v < n) dist[v] = bad ? 0u : LIVE_FAR;
    const unsigned long long b = __ballot(bad);
    if (b && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) {   // (the first bad lane of a wavefront holds its least root)
        atomicAdd(&lc->fair_components, (unsigned long long)__popcll(b));
        atomicMin(&lc->first_root, (unsigned)v);
    }
}

// ---- reach (mc_engine_liveness_check): from which states of M is a violating component reached inside M, and how far is it
struct LiveCheckCounters {
    unsigned long long mask_states, bad_starts;
    unsigned witness, pad;   // the least S state with a dist, ~0u = none
};
// the other states of the violating components (k_live_verdict<true> marked their roots; a root keeps its value: no lane writes what
// another reads)
static __global__ void __launch_bounds__(256)
k_live_reach_init(uint64_t n, const uint32_t *__restrict__ scc, const uint32_t *__restrict__ pred, LiveCheck ck, uint32_t *dist) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n || !live_passable(ck, pred[v])) return;
    const uint32_t r = scc[v];
    if (r != (uint32_t)v && r < n && dist[r] == 0u) dist[v] = 0u;
}
// one sweep, in place: a lane may read a dist another lane lowered in the same sweep — values only fall, towards the one fixed point
static __global__ void __launch_bounds__(256)
k_live_reach(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, const uint32_t *__restrict__ pred, LiveCheck ck,
             uint32_t *dist, unsigned *flag) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool changed = false;
    if (v < n && live_passable(ck, pred[v])) {
        const uint32_t mine = dist[v];
        if (mine != 0u) {
            const uint64_t o = offsets[v];
            const uint32_t best = live_reach_step((uint32_t)v, mine, dst + o, offsets[v + 1] - o, dist,
                                                  [&](uint32_t d) { return d < n && live_passable(ck, pred[d]); });
            if (best < mine) { dist[v] = best; changed = true; }
        }
    }
    live_raise(changed, flag);
}
static __global__ void __launch_bounds__(256)
k_live_witness(uint64_t n, const uint32_t *__restrict__ pred, LiveCheck ck, const uint32_t *__restrict__ dist, uint64_t init_states,
               LiveCheckCounters *cc) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t bits = v < n ? pred[v] : 0u;
    const bool in_m = v < n && live_in_mask(ck, bits);
    const bool bad = in_m && dist[v] != LIVE_FAR && live_in_start(ck, bits, v < init_states);
    const unsigned long long m = __ballot(in_m), b = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cc->mask_states, (unsigned long long)__popcll(m));
    if (b && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) {   // (the first bad lane of a wavefront holds its least state)
        atomicAdd(&cc->bad_starts, (unsigned long long)__popcll(b));
        atomicMin(&cc->witness, (unsigned)v);
    }
}

// ---- strong fairness (mc_engine_liveness_strong / mc_engine_liveness_check_strong): the refinement of liveness.h
struct LiveStrongCounters {
    unsigned long long closed, final_components;   // states closed so far; final violating components so far
    unsigned first_root, open;                     // the least final root, ~0u = none; some state is still open (cleared per round)
};
// every state of M is open, the others closed; a closed state's refined id is its own index
template <bool MASKED>
static __global__ void __launch_bounds__(256)
k_live_open_init(uint64_t n, const uint32_t *__restrict__ pred, LiveCheck ck, uint8_t *__restrict__ open, uint32_t *__restrict__ fscc,
                 uint32_t *__restrict__ fsize) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    open[v] = !MASKED || live_in_mask(ck, pred[v]) ? LIVE_ST_OPEN : LIVE_ST_CLOSED;
    fscc[v] = (uint32_t)v;
    fsize[v] = 1u;
}
// the open-set build, beside k_scc_mask: scc[] is all SCC_LIVE when this runs; a state that is not open is a component of its own
static __global__ void __launch_bounds__(256)
k_scc_open(uint64_t n, const uint8_t *__restrict__ open, uint32_t *__restrict__ scc) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n && open[v] != LIVE_ST_OPEN) scc[v] = (uint32_t)v;
}
// en of every open state (the whole row: the full graph's), OR-ed into enabled[] at the state's component of the round; k_live_reduce's
// merge.  The entries were cleared before the launch.
template <bool UNITS>
__device__ __forceinline__ void
live_enabled_body(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, const int8_t *__restrict__ proc,
                  const uint32_t *__restrict__ scc, const uint32_t *__restrict__ size, const uint8_t *__restrict__ open, unsigned long long *enabled,
                  const uint64_t *of_unit) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = v < n && open[v] == LIVE_ST_OPEN;
    uint64_t en = 0;
    uint32_t comp = 0;
    if (active) {
        const uint64_t o = offsets[v];
        if constexpr (UNITS) en = live_enabled_in_units((uint32_t)v, dst + o, proc + o, offsets[v + 1] - o, scc, of_unit);
        else en = live_enabled_in((uint32_t)v, dst + o, proc + o, offsets[v + 1] - o, scc);
        comp = scc[v];
    }
    const bool alone = active && size[comp] == 1;
    if (alone) enabled[comp] = en;
    unsigned long long rest = __ballot(active && !alone);
    const unsigned lane = threadIdx.x & 63;
    while (rest) {   // (the loop's condition is the same in every lane)
        const int lead = __ffsll((long long)rest) - 1;
        const uint32_t c0 = (uint32_t)__shfl((int)comp, lead);
        const bool same = active && !alone && comp == c0;
        const unsigned long long e = wave_or_u64(same ? en : 0ull);
        if ((int)lane == lead && e) atomicOr(&enabled[c0], e);
        rest &= ~__ballot(same);
    }
}
static __global__ void __launch_bounds__(256)
k_live_enabled(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, const int8_t *__restrict__ proc,
               const uint32_t *__restrict__ scc, const uint32_t *__restrict__ size, const uint8_t *__restrict__ open, unsigned long long *enabled) {
    live_enabled_body<false>(n, offsets, dst, proc, scc, size, open, enabled, nullptr);
}
static __global__ void __launch_bounds__(256)
k_live_enabled_units(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, const int8_t *__restrict__ unit,
                     const uint32_t *__restrict__ scc, const uint32_t *__restrict__ size, const uint8_t *__restrict__ open, unsigned long long *enabled,
                     const uint64_t *__restrict__ of_unit) {
    __shared__ uint64_t tab[LIVE_UNIT_TAB];
    live_stage_units(of_unit, tab);
    live_enabled_body<true>(n, offsets, dst, unit, scc, size, open, enabled, tab);
}
// has_target of a component: the property checks keep "holds a T state" in done[]; Termination keeps "holds a Done state", and T is
// "not Done" (a Done state is absorbing: a component with one is that one state)
__device__ __forceinline__ bool live_strong_target(bool term, unsigned done) { return term ? done == 0u : done != 0u; }
// per root of an open component: the final violating ones, counted, and the least of them
static __global__ void __launch_bounds__(256)
k_live_classify(uint64_t n, const uint32_t *__restrict__ scc, const uint32_t *__restrict__ size, const uint8_t *__restrict__ open,
                const unsigned long long *__restrict__ taken, const unsigned long long *__restrict__ disabled, const unsigned *__restrict__ done,
                const unsigned long long *__restrict__ enabled, uint64_t all, uint64_t weak, uint64_t strong, bool term, LiveStrongCounters *sc) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = v < n && open[v] == LIVE_ST_OPEN && scc[v] == (uint32_t)v;
    const bool bad = root && live_violates_strong(all, weak, strong, taken[v], disabled[v], enabled[v], live_strong_target(term, done[v]), size[v]);
    const unsigned long long b = __ballot(bad);
    if (b && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) {   // (the first bad lane of a wavefront holds its least root)
        atomicAdd(&sc->final_components, (unsigned long long)__popcll(b));
        atomicMin(&sc->first_root, (unsigned)v);
    }
}
// per open state: closed, kept open or final, by plain stores to its own entries; dist (property checks; null for Termination) is 0 in
// a final component
template <bool UNITS>
__device__ __forceinline__ void
live_refine_body(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, const int8_t *__restrict__ proc,
                 const uint32_t *__restrict__ scc, const uint32_t *__restrict__ size, const unsigned long long *__restrict__ taken,
                 const unsigned long long *__restrict__ disabled, const unsigned *__restrict__ done, const unsigned long long *__restrict__ enabled,
                 uint64_t all, uint64_t weak, uint64_t strong, bool term, uint8_t *open, uint32_t *__restrict__ fscc, uint32_t *__restrict__ fsize,
                 uint32_t *__restrict__ dist, LiveStrongCounters *sc, const uint64_t *of_unit) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = v < n && open[v] == LIVE_ST_OPEN;
    uint8_t next = LIVE_ST_CLOSED;
    if (active) {
        const uint32_t c = scc[v];
        const uint64_t tk = taken[c], en_c = enabled[c], o = offsets[v];
        const int cls = live_classify(all, weak, strong, tk, disabled[c], en_c, live_strong_target(term, done[c]), size[c]);
        uint64_t en;
        if constexpr (UNITS) en = live_enabled_in_units((uint32_t)v, dst + o, proc + o, offsets[v + 1] - o, scc, of_unit);
        else en = live_enabled_in((uint32_t)v, dst + o, proc + o, offsets[v + 1] - o, scc);
        next = live_refine_state(cls, live_blockers(all, strong, en_c, tk), en);
        open[v] = next;
        if (next == LIVE_ST_FINAL) {
            fscc[v] = c;
            fsize[v] = size[c];
            if (dist) dist[v] = 0u;
        }
    }
    const unsigned long long closing = __ballot(active && next == LIVE_ST_CLOSED), staying = __ballot(active && next == LIVE_ST_OPEN);
    if ((threadIdx.x & 63) == 0) {
        if (closing) atomicAdd(&sc->closed, (unsigned long long)__popcll(closing));
        if (staying) atomicOr(&sc->open, 1u);
    }
}
static __global__ void __launch_bounds__(256)
k_live_refine(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, const int8_t *__restrict__ proc,
              const uint32_t *__restrict__ scc, const uint32_t *__restrict__ size, const unsigned long long *__restrict__ taken,
              const unsigned long long *__restrict__ disabled, const unsigned *__restrict__ done, const unsigned long long *__restrict__ enabled,
              uint64_t all, uint64_t weak, uint64_t strong, bool term, uint8_t *open, uint32_t *__restrict__ fscc, uint32_t *__restrict__ fsize,
              uint32_t *__restrict__ dist, LiveStrongCounters *sc) {
    live_refine_body<false>(n, offsets, dst, proc, scc, size, taken, disabled, done, enabled, all, weak, strong, term, open, fscc, fsize, dist, sc, nullptr);
}
static __global__ void __launch_bounds__(256)
k_live_refine_units(uint64_t n, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ dst, const int8_t *__restrict__ unit,
                    const uint32_t *__restrict__ scc, const uint32_t *__restrict__ size, const unsigned long long *__restrict__ taken,
                    const unsigned long long *__restrict__ disabled, const unsigned *__restrict__ done, const unsigned long long *__restrict__ enabled,
                    uint64_t all, uint64_t weak, uint64_t strong, bool term, uint8_t *open, uint32_t *__restrict__ fscc, uint32_t *__restrict__ fsize,
                    uint32_t *__restrict__ dist, LiveStrongCounters *sc, const uint64_t *__restrict__ of_unit) {
    __shared__ uint64_t tab[LIVE_UNIT_TAB];
    live_stage_units(of_unit, tab);
    live_refine_body<true>(n, offsets, dst, unit, scc, size, taken, disabled, done, enabled, all, weak, strong, term, open, fscc, fsize, dist, sc, tab);
}

// ---- the scans (state_graph.h declares them)
// degree (32 bits) as the scan's 64-bit input: the offsets of a graph of more than 2^32 edges do not wrap
struct ScanU32ToU64 {
    __host__ __device__ __forceinline__ uint64_t operator()(const uint32_t &d) const { return (uint64_t)d; }
};
int scan_exclusive_u32_to_u64(const uint32_t *in, uint64_t *out, uint64_t n, DevBuf<char> &tmp, hipStream_t stream, const char *call) {
    hipcub::TransformInputIterator<uint64_t, ScanU32ToU64, const uint32_t *> it(in, ScanU32ToU64());
    size_t need = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, it, out, (int)n, stream));
    if (int rc = graph_alloc(tmp, need, "the scan", call)) return rc;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, need, it, out, (int)n, stream));
    return MC_OK;
}
// a rank's answers (one byte per candidate, non-zero = keep) as the 0 / 1 the sum counts
struct ScanAnswerBit {
    __host__ __device__ uint32_t operator()(const uint8_t &a) const { return a ? 1u : 0u; }
};
int scan_answers_inclusive(const uint8_t *answers, uint32_t *incl, uint64_t n, DevBuf<char> &tmp, hipStream_t stream) {
    hipcub::TransformInputIterator<uint32_t, ScanAnswerBit, const uint8_t *> it(answers, ScanAnswerBit());
    size_t need = 0;
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, need, it, incl, (int)n, stream));
    HIP_TRY(tmp.reserve(need));
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(tmp.p, need, it, incl, (int)n, stream));
    return MC_OK;
}

}  // namespace mc

#endif  // TLAMC_ENGINE_LIVE_H
