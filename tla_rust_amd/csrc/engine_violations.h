// engine_violations.h — the DEVICE half of TLC's -continue (MC_F_CONTINUE, mc_engine_violations): two passes over a FLAGGED BFS level (one
// after which DevCounters::viol_key is set), which say what the level's single minimum key cannot: how many stored states break which
// invariant, how many expanded states are deadlocked, how many violating successors lie outside the model, and whether a fatal kind (a
// failed Assert, an evaluation error) is among them.  Included by engine.hip only, after engine_kernels.h (arena_cref, the wave
// reductions, viol_key, stored_state_status, ChecksOnExpand).  The rules are violations.h's, MC_HD code the host runs too.
//
// Both kernels keep, per workgroup, a histogram and a 64-bit minimum per cell in LDS (2 columns x VIOL_BINS bins: column 0 = stored
// states / deadlocked states with the smallest arena index, column 1 = successors outside the model / failing pairs with the smallest
// violation key) and flush each non-empty cell with one global atomicAdd and one global atomicMin at their end.  They store nothing
// else: no seen-set access, no write to DevCounters, no state.  A level without a violation launches neither.
#ifndef TLAMC_ENGINE_VIOLATIONS_H
#define TLAMC_ENGINE_VIOLATIONS_H

#include "violations.h"

namespace mc {

constexpr int VIOL_CELLS = 2 * VIOL_BINS;
struct ViolBins {   // the device table a run accumulates; cell = column * VIOL_BINS + bin
    unsigned long long count[VIOL_CELLS];
    unsigned long long first[VIOL_CELLS];   // ~0 = none
};
struct ViolLds {
    unsigned cnt[VIOL_CELLS];
    unsigned long long mn[VIOL_CELLS];
};

__device__ __forceinline__ void viol_zero(ViolLds &L) {
    for (int i = (int)threadIdx.x; i < VIOL_CELLS; i += (int)blockDim.x) { L.cnt[i] = 0; L.mn[i] = ~0ull; }
    __syncthreads();
}
// The lanes of a wavefront with `on` set count themselves into `cell` and offer `key` to its minimum.  Every lane of the wavefront calls
// it (ballots, shuffles).  Where the lanes agree on the cell, one lane adds popcount(ballot) and carries the wavefront's minimum; else
// every lane does its own two LDS atomics.
__device__ __forceinline__ void viol_note(ViolLds &L, bool on, int cell, unsigned long long key) {
    on = on && cell >= 0 && cell < VIOL_CELLS;   // (a cell outside the table would show as a count that is not the reference's; never as a stray write)
    const unsigned long long b = __ballot(on);
    if (!b) return;
    const int lead = __ffsll((long long)b) - 1;
    const int cell0 = __shfl(cell, lead);
    if (__ballot(on && cell != cell0) == 0) {   // (wave-uniform: every lane takes the same branch)
        const unsigned long long m = wave_min_u64(on ? key : ~0ull);
        if ((int)(threadIdx.x & 63) == lead) {
            atomicAdd(&L.cnt[cell0], (unsigned)__popcll(b));
            atomicMin(&L.mn[cell0], m);
        }
    } else if (on) {
        atomicAdd(&L.cnt[cell], 1u);
        atomicMin(&L.mn[cell], key);
    }
}
__device__ __forceinline__ void viol_flush(const ViolLds &L, ViolBins *bins) {
    __syncthreads();
    for (int i = (int)threadIdx.x; i < VIOL_CELLS; i += (int)blockDim.x)
        if (L.cnt[i]) {
            atomicAdd(&bins->count[i], (unsigned long long)L.cnt[i]);
            atomicMin(&bins->first[i], L.mn[i]);
        }
}

// One lane per stored state of [lo, hi): the invariant it is listed under (viol_stored_bin) bumps column 0 of that bin, with the
// state's arena index.  A lowering that checks stored states evaluates the state itself; the others the (parent, slot) pair of its
// trace record, or Init's status for a state without a parent.
template <class S>
__global__ void __launch_bounds__(256)
k_viol_stored(typename S::Params prm, const uint64_t *__restrict__ arena, const uint32_t *__restrict__ parent, const uint16_t *__restrict__ pslot,
              uint64_t lo, uint64_t hi, ViolBins *__restrict__ bins) {
    __shared__ ViolLds L;
    viol_zero(L);
    const uint64_t idx = lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = idx < hi;   // (no lane leaves before the flush: the barriers are the workgroup's)
    int bin = -1;
    if (active) {
        const int W = S::words(prm);
        const CWordRef self = arena_cref(arena, idx, W);
        uint32_t p = 0xffffffffu;
        if constexpr (!ChecksOnExpand<S>::value) p = parent[idx];
        const bool has_parent = p != 0xffffffffu;
        if (!has_parent || p < idx)   // (a parent lies below its successors in the arena; a record that cannot be one is counted nowhere)
            bin = viol_stored_bin<S>(prm, self, has_parent, ViolModel<S>::ninv(prm),
                [&]() -> unsigned {
                    if constexpr (ChecksOnExpand<S>::value) {
                        typename S::Local loc;
                        S::load(prm, self, loc);
                        return stored_state_status<S>(prm, loc, self);
                    } else return 0u;
                },
                [&]() -> unsigned {
                    const CWordRef ps = arena_cref(arena, p, W);
                    typename S::Local loc;
                    S::load(prm, ps, loc);
                    uint64_t f = 0;
                    return S::eval(prm, loc, ps, (int)pslot[idx], f);
                });
    }
    viol_note(L, active && bin >= 0, bin, idx);
    viol_flush(L, bins);
}

// One lane per expanded state of the chunk [lo, hi) (columns as in k_expand / k_coverage_generated), the slot loop to the wavefront's
// largest nslots: successors outside the model that break an invariant (column 1 of the invariant's bin), the pairs that end the
// search (column 1 of the fatal bin), both with the engine's violation key; then the deadlocked states (column 0 of the deadlock bin).
template <class S>
__global__ void __launch_bounds__(256)
k_viol_frontier(typename S::Params prm, const uint64_t *__restrict__ arena, uint64_t lo, uint64_t hi, uint64_t ncols, unsigned flags,
                ViolBins *__restrict__ bins) {
    __shared__ ViolLds L;
    viol_zero(L);
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
    unsigned gen = 0;
    for (int slot = 0; slot < wns; ++slot) {
        ViolPair r{VIOL_P_NONE, 0u, 0u, 0u, false};
        if (slot < ns) {
            uint64_t f = 0;
            const unsigned st = S::eval(prm, loc, s, slot, f);
            if (st & ST_ENABLED) ++gen;
            r = viol_pair<S>(st, ViolModel<S>::ninv(prm));   // (an index behind the model's invariants: a property of the step, fatal)
        }
        const unsigned long long key = viol_key(idx, (unsigned)slot, r.kind, r.inv);
        const int column = viol_pair_column(r);
        viol_note(L, column >= 0, column * VIOL_BINS + (int)r.bin, key);
        viol_note(L, viol_ends_search(r), VIOL_BINS + VIOL_BIN_FATAL, key);
    }
    viol_note(L, active && viol_deadlocked(gen, (flags & MC_F_DEADLOCK) != 0), VIOL_BIN_DEADLOCK, idx);
    viol_flush(L, bins);
}

static __global__ void k_clear_viol_key(DevCounters *ctr) { ctr->viol_key = ~0ull; }

}  // namespace mc

#endif  // TLAMC_ENGINE_VIOLATIONS_H
