// engine_coverage.h — the DEVICE half of TLC's -coverage (MC_F_COVERAGE, mc_engine_coverage): two histogram kernels over what a BFS
// level expanded and what it added.  Included by engine.hip only (inside namespace mc, after engine_kernels.h: arena_cref, the wave
// reductions).  What counts and which action a (state, slot) pair belongs to is coverage.h's, MC_HD code the host runs too.
//
// Both kernels keep a per-workgroup histogram in LDS (bin 0 = Init, bin a + 1 = action id a; at most COV_MAX_BINS bins) and flush its
// non-zero bins with one 64-bit global atomicAdd each at their end: a workgroup of 256 states issues as many global atomics as the level
// has live actions, not one per successor.  They store nothing else: no seen-set access, no violation key, no counter of the search.
#ifndef TLAMC_ENGINE_COVERAGE_H
#define TLAMC_ENGINE_COVERAGE_H

#include "coverage.h"

namespace mc {

// The states [lo, hi) in the chunks the expand kernel saw: f(c0, c1, ncols), column 0 = the 64-aligned state at or below c0.  Host code:
// how the engine launches every kernel that takes (lo, hi, ncols) — the two here, k_viol_frontier, the graph passes.  chunk: a multiple
// of 64, at least 64.
template <class F>
inline void each_chunk(uint64_t lo, uint64_t hi, uint64_t chunk, F &&f) {
    for (uint64_t c0 = lo; c0 < hi;) {
        const uint64_t base = c0 & ~63ull;
        const uint64_t c1 = base + chunk < hi ? base + chunk : hi;
        f(c0, c1, ((c1 - base) + 63) & ~63ull);
        c0 = c1;
    }
}

// One bump of the workgroup's histogram by the lanes of a wavefront with `on` set, each for its bin `bin`.  Every lane of the wavefront
// calls it (the shuffle and the ballots are wavefront operations).  Where the lanes agree on the bin — always when the action is a
// function of the slot, often otherwise — one lane adds popcount(ballot); else every lane does its own LDS atomic add.
__device__ __forceinline__ void cov_bump(unsigned *hist, int nbins, bool on, int bin) {
    on = on && bin >= 0 && bin < nbins;   // (an id outside the model's range would show as a sum that is not mc_result's; never as a stray write)
    const unsigned long long b = __ballot(on);
    if (!b) return;
    const int lead = __ffsll((long long)b) - 1;
    const int bin0 = __shfl(bin, lead);
    if (__ballot(on && bin != bin0) == 0) {
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(&hist[bin0], (unsigned)__popcll(b));
    } else if (on) {
        atomicAdd(&hist[bin], 1u);
    }
}
__device__ __forceinline__ void cov_zero(unsigned *hist, int nbins) {
    for (int i = (int)threadIdx.x; i < nbins; i += (int)blockDim.x) hist[i] = 0;
    __syncthreads();
}
__device__ __forceinline__ void cov_flush(const unsigned *hist, int nbins, unsigned long long *bins) {
    __syncthreads();
    for (int i = (int)threadIdx.x; i < nbins; i += (int)blockDim.x)
        if (hist[i]) atomicAdd(&bins[i], (unsigned long long)hist[i]);
}

// generated[a]: one lane per frontier state of the chunk [lo, hi) (columns as in k_expand: column 0 = the 64-aligned state below lo),
// the slot loop to the wavefront's largest nslots; every pair that counts (cov_counts) bumps its action's bin.
template <class S>
__global__ void __launch_bounds__(256)
k_coverage_generated(typename S::Params prm, const uint64_t *__restrict__ arena, uint64_t lo, uint64_t hi, uint64_t ncols,
                     unsigned long long *__restrict__ bins, int nbins) {
    __shared__ unsigned hist[COV_MAX_BINS];
    cov_zero(hist, nbins);
    const uint64_t col = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t idx = (lo & ~63ull) + col;
    const bool active = col < ncols && idx >= lo && idx < hi;   // (no lane leaves before the flush: the barriers are the workgroup's)
    const CWordRef s = arena_cref(arena, active ? idx : lo, S::words(prm));
    typename S::Local loc;
    int ns = 0;
    if (active) {
        S::load(prm, s, loc);
        ns = S::nslots(prm, loc);
    }
    const int wns = (int)wave_max_u32((unsigned)ns);
    for (int slot = 0; slot < wns; ++slot) {
        bool on = false;
        int a = -1;
        if (slot < ns) {
            uint64_t f = 0;
            on = cov_counts(S::eval(prm, loc, s, slot, f));
            if (on) a = CovAction<S>::of(prm, loc, s, slot);
        }
        cov_bump(hist, nbins, on, a + 1);
    }
    cov_flush(hist, nbins, bins);
}

// distinct[a]: one lane per state of [lo, hi), the states a level added (or Init): its trace record (parent index, slot) names the pair
// that was first to find it; the parent row is loaded and the pair's action taken as above.  A state without a parent is an initial one.
template <class S>
__global__ void __launch_bounds__(256)
k_coverage_distinct(typename S::Params prm, const uint64_t *__restrict__ arena, const uint32_t *__restrict__ parent,
                    const uint16_t *__restrict__ pslot, uint64_t lo, uint64_t hi, unsigned long long *__restrict__ bins, int nbins) {
    __shared__ unsigned hist[COV_MAX_BINS];
    cov_zero(hist, nbins);
    const uint64_t idx = lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = idx < hi;
    int bin = 0;
    if (active) {
        const uint32_t p = parent[idx];
        if (p != 0xffffffffu && p < idx) {   // (a parent lies below its successors in the arena)
            const CWordRef s = arena_cref(arena, p, S::words(prm));
            typename S::Local loc;
            if constexpr (!CovAction<S>::BY_SLOT) S::load(prm, s, loc);
            bin = CovAction<S>::of(prm, loc, s, (int)pslot[idx]) + 1;
        } else if (p != 0xffffffffu) {
            bin = -1;   // a record that cannot be one (never written by the engine): cov_bump drops bin -1, so it is counted nowhere and
                        // shows as a sum below mc_result.distinct instead of as a read outside the states written so far
        }
    }
    cov_bump(hist, nbins, active, bin);
    cov_flush(hist, nbins, bins);
}

}  // namespace mc

#endif  // TLAMC_ENGINE_COVERAGE_H
