// engine_graph.h — the DEVICE half of the state graph (mc_engine_graph): the edge list of the reachable graph in CSR form, built after a
// search from what it left resident — the arena's rows and the seen-set's fingerprints.  Included by engine.hip only (inside namespace
// mc, after engine_kernels.h: arena_cref, the wave reductions, SEEN_SPARSE).  What a (state, slot) pair contributes and how a key is
// looked up is graph.h's, MC_HD code the host runs too.
//
//   k_graph_index    one lane per stored state: slot_index[position of the state's key in the seen-set] = its arena index.  The side
//                    array has one 32-bit entry per seen-set slot, so "fingerprint -> arena index" is the seen-set's own probe plus one
//                    4-byte read: no second hash table, no second placement rule.
//   k_graph_degree   pass 1, one lane per expanded state: the slot loop to the wavefront's largest nslots, degree[i] = its edges
//   k_graph_fill     pass 2, the same loop: dst[offsets[i] + k], act[offsets[i] + k] in slot order
//   k_live_proc      the loop a third time, for mc_engine_liveness: proc[offsets[i] + k] beside act[] (LiveProc<S>, liveness.h)
//   k_live_unit      and a fourth time, for mc_engine_liveness_units: unit[offsets[i] + k], from the slot's instance and the label it stands at
//   k_live_pred      one lane per stored state, the same chunks: pred[i] = the state predicates of the cfg's temporal properties that hold
//                    in it, one bit each (LivePred<S>, liveness.h)
// Between the passes an exclusive scan turns degree into offsets.  Nothing here writes the arena, the seen-set or a counter of the search.
// These are the kernels that know the lowering; whatever consumes the CSR arrays alone is compiled once, in state_graph.hip.
#ifndef TLAMC_ENGINE_GRAPH_H
#define TLAMC_ENGINE_GRAPH_H

#include "liveness.h"   // (graph.h, and LiveProc<S>)

namespace mc {

static_assert(GRAPH_SEEN_SPARSE == SEEN_SPARSE, "graph.h reads the seen-set in the form the search kernels write it");

constexpr uint32_t GRAPH_NO_INDEX = 0xffffffffu;   // a slot_index entry no stored state has claimed
constexpr unsigned GRAPH_SLOT_SELF = 0xffffu;      // GraphCounters::first_bad: the state's OWN key is missing (no slot)

struct GraphCounters {
    unsigned long long missing_states;   // stored states whose own key the seen-set does not hold
    unsigned long long missing_succ;     // unflagged, in-model successors absent from the seen-set (or from slot_index)
    unsigned long long first_bad;        // the least (state index << 16 | slot) of the two kinds; ~0 = none
    unsigned long long dropped, self_loops;
    unsigned max_degree, pad;
};
MC_HD unsigned long long graph_bad_key(uint64_t idx, unsigned slot) { return ((unsigned long long)idx << 16) | (slot & 0xffffu); }

template <class S>
__global__ void __launch_bounds__(256)
k_graph_index(typename S::Params prm, const uint64_t *__restrict__ arena, uint64_t n, const uint64_t *__restrict__ table, uint64_t seen,
              uint32_t *__restrict__ slot_index, uint64_t nslots_total, GraphCounters *gc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t pos = seen_find(table, seen, S::fp_of(prm, arena_cref(arena, i, S::words(prm))));
    if (pos < nslots_total) {
        slot_index[pos] = (uint32_t)i;
    } else {   // two different states with one fingerprint would not get here (the second is never stored): the arena and the table disagree
        atomicAdd(&gc->missing_states, 1ull);
        atomicMin(&gc->first_bad, graph_bad_key(i, GRAPH_SLOT_SELF));
    }
}

// The two passes share the walk: one lane per state of the chunk [lo, hi) (columns as in k_expand: column 0 = the 64-aligned state
// below lo, so lo need not be a multiple of 64), every lane of a wavefront in the slot loop to the wavefront's largest nslots.
// FILL = false: count; FILL = true: write.
template <class S, bool FILL>
__device__ __forceinline__ void graph_walk(const typename S::Params &prm, const uint64_t *__restrict__ arena, uint64_t lo, uint64_t hi,
                                           uint64_t ncols, const uint64_t *__restrict__ table, uint64_t seen,
                                           const uint32_t *__restrict__ slot_index, uint64_t nslots_total, uint32_t *__restrict__ degree,
                                           const uint64_t *__restrict__ offsets, uint32_t *__restrict__ dst, int16_t *__restrict__ act,
                                           GraphCounters *gc) {
    const uint64_t col = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t idx = (lo & ~63ull) + col;
    const bool active = col < ncols && idx >= lo && idx < hi;
    const CWordRef s = arena_cref(arena, active ? idx : lo, S::words(prm));
    typename S::Local loc;
    int ns = 0;
    if (active) {
        S::load(prm, s, loc);
        ns = S::nslots(prm, loc);
    }
    const int wns = (int)wave_max_u32((unsigned)ns);
    unsigned deg = 0, dropped = 0, selfs = 0, missing = 0;
    unsigned long long bad = ~0ull;
    uint64_t out = 0, end = 0;
    if (FILL && active) { out = offsets[idx]; end = offsets[idx + 1]; }
    for (int slot = 0; slot < wns; ++slot) {
        if (slot >= ns) continue;   // (no wavefront operation inside the loop)
        uint64_t f = 0, pos;
        const unsigned kind = graph_edge(S::eval(prm, loc, s, slot, f), f, table, seen, pos);
        if (kind == GE_SELF || kind == GE_EDGE) {
            if constexpr (FILL) {
                uint32_t to = (uint32_t)idx;
                if (kind == GE_EDGE) {
                    to = pos < nslots_total ? slot_index[pos] : GRAPH_NO_INDEX;
                    if (to == GRAPH_NO_INDEX) { ++missing; bad = min(bad, graph_bad_key(idx, (unsigned)slot)); }   // a key nobody stored a state for
                }
                selfs += to == (uint32_t)idx ? 1u : 0u;   // (a stuttering step, or a successor whose key is the state's own)
                if (out + deg < end) {   // (pass 1 counted this edge: the bound holds; it is checked so that a disagreement can never write outside the row)
                    dst[out + deg] = to;
                    act[out + deg] = (int16_t)CovAction<S>::of(prm, loc, s, slot);
                }
            }
            ++deg;
        } else if (kind == GE_DROPPED) {
            ++dropped;
        } else if (kind == GE_MISSING) {
            ++missing;
            bad = min(bad, graph_bad_key(idx, (unsigned)slot));
        }
    }
    if (!FILL && active) degree[idx] = deg;
    // pass 1 owns the statistics; pass 2 reports what it alone can see: a key without an arena index, and the edges that end where they start
    const unsigned wmiss = wave_sum_u32(missing);
    const unsigned long long wbad = wave_min_u64(bad);
    const unsigned wdrop = FILL ? 0u : wave_sum_u32(dropped), wself = FILL ? wave_sum_u32(selfs) : 0u, wmax = FILL ? 0u : wave_max_u32(deg);
    if ((threadIdx.x & 63) == 0) {
        if (wmiss) { atomicAdd(&gc->missing_succ, (unsigned long long)wmiss); atomicMin(&gc->first_bad, wbad); }
        if (wdrop) atomicAdd(&gc->dropped, (unsigned long long)wdrop);
        if (wself) atomicAdd(&gc->self_loops, (unsigned long long)wself);
        if (wmax) atomicMax(&gc->max_degree, wmax);
    }
}

template <class S>
__global__ void __launch_bounds__(256)
k_graph_degree(typename S::Params prm, const uint64_t *__restrict__ arena, uint64_t lo, uint64_t hi, uint64_t ncols,
               const uint64_t *__restrict__ table, uint64_t seen, uint32_t *__restrict__ degree, GraphCounters *gc) {
    graph_walk<S, false>(prm, arena, lo, hi, ncols, table, seen, nullptr, 0, degree, nullptr, nullptr, nullptr, gc);
}
template <class S>
__global__ void __launch_bounds__(256)
k_graph_fill(typename S::Params prm, const uint64_t *__restrict__ arena, uint64_t lo, uint64_t hi, uint64_t ncols,
             const uint64_t *__restrict__ table, uint64_t seen, const uint32_t *__restrict__ slot_index, uint64_t nslots_total,
             const uint64_t *__restrict__ offsets, uint32_t *__restrict__ dst, int16_t *__restrict__ act, GraphCounters *gc) {
    graph_walk<S, true>(prm, arena, lo, hi, ncols, table, seen, slot_index, nslots_total, nullptr, offsets, dst, act, gc);
}

// proc[] beside act[]: graph_walk's loop once more (the chunks, the columns, the wavefront's largest nslots, graph_edge), writing the
// process instance of every counted slot at the edge's place
template <class S>
__global__ void __launch_bounds__(256)
k_live_proc(typename S::Params prm, const uint64_t *__restrict__ arena, uint64_t lo, uint64_t hi, uint64_t ncols,
            const uint64_t *__restrict__ table, uint64_t seen, const uint64_t *__restrict__ offsets, int8_t *__restrict__ proc) {
    const uint64_t col = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t idx = (lo & ~63ull) + col;
    const bool active = col < ncols && idx >= lo && idx < hi;
    const CWordRef s = arena_cref(arena, active ? idx : lo, S::words(prm));
    typename S::Local loc;
    int ns = 0;
    uint64_t out = 0, end = 0;
    if (active) {
        S::load(prm, s, loc);
        ns = S::nslots(prm, loc);
        out = offsets[idx];
        end = offsets[idx + 1];
    }
    const int wns = (int)wave_max_u32((unsigned)ns);
    for (int slot = 0; slot < wns; ++slot) {
        if (slot >= ns) continue;   // (no wavefront operation inside the loop)
        uint64_t f = 0, pos;
        const unsigned kind = graph_edge(S::eval(prm, loc, s, slot, f), f, table, seen, pos);
        if (kind != GE_SELF && kind != GE_EDGE) continue;
        if (out < end) proc[out] = (int8_t)LiveProc<S>::of(prm, slot);
        ++out;
    }
}

// unit[] beside proc[] (mc_engine_liveness_units): the same walk and the same graph_edge decisions; the unit of an
// edge is a function of the instance of the slot and of the label that instance stands at in the row the walk has loaded (the SOURCE
// state), read from the (instance, label) -> unit table in device memory
template <class S>
__global__ void __launch_bounds__(256)
k_live_unit(typename S::Params prm, const uint64_t *__restrict__ arena, uint64_t lo, uint64_t hi, uint64_t ncols,
            const uint64_t *__restrict__ table, uint64_t seen, const uint64_t *__restrict__ offsets, LiveUnitTab tab, int8_t *__restrict__ unit) {
    const uint64_t col = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t idx = (lo & ~63ull) + col;
    const bool active = col < ncols && idx >= lo && idx < hi;
    const CWordRef s = arena_cref(arena, active ? idx : lo, S::words(prm));
    typename S::Local loc;
    int ns = 0;
    uint64_t out = 0, end = 0;
    if (active) {
        S::load(prm, s, loc);
        ns = S::nslots(prm, loc);
        out = offsets[idx];
        end = offsets[idx + 1];
    }
    const int wns = (int)wave_max_u32((unsigned)ns);
    for (int slot = 0; slot < wns; ++slot) {
        if (slot >= ns) continue;   // (no wavefront operation inside the loop)
        uint64_t f = 0, pos;
        const unsigned kind = graph_edge(S::eval(prm, loc, s, slot, f), f, table, seen, pos);
        if (kind != GE_SELF && kind != GE_EDGE) continue;
        if (out < end) unit[out] = (int8_t)live_edge_unit<S>(prm, loc, tab, slot);
        ++out;
    }
}

// pred[] for mc_engine_predicates / mc_engine_liveness_check: the arena row loaded as the walk loads it, every predicate of `tab` run on
// it.  An evaluation error is no value: the least (state << 8 | predicate) of them is left in *first_bad (~0 = none).
template <class S>
__global__ void __launch_bounds__(256)
k_live_pred(typename S::Params prm, const uint64_t *__restrict__ arena, uint64_t lo, uint64_t hi, uint64_t ncols,
            const uint64_t *__restrict__, uint64_t, LivePredTab tab, uint32_t *__restrict__ pred, unsigned long long *first_bad) {
    const uint64_t col = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t idx = (lo & ~63ull) + col;
    if (!(col < ncols && idx >= lo && idx < hi)) return;
    typename S::Local loc;
    S::load(prm, arena_cref(arena, idx, S::words(prm)), loc);
    uint32_t bits = 0;
    for (int k = 0; k < tab.n && k < LIVE_MAX_PREDS; ++k) {
        int32_t res = 0;
        if (!LivePred<S>::eval(prm, loc, tab, k, res)) { atomicMin(first_bad, (unsigned long long)idx << 8 | (unsigned)k); continue; }
        if (res) bits |= 1u << k;
    }
    pred[idx] = bits;
}

}  // namespace mc

#endif  // TLAMC_ENGINE_GRAPH_H
