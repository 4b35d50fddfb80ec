// engine_behaviours.h — the DEVICE half of behaviour checking (mc_engine_behaviours): k_behaviours, one wavefront per
// recorded behaviour, one lane per candidate state.  Included by engine.hip only (after engine_kernels.h: arena_ref / arena_cref, the
// wave reductions).  The rule is behaviour.h's; this file is how 64 lanes apply it.
//
// A round of behaviours b0 .. b0+n-1 runs as n workgroups of ONE wavefront each: behaviours differ in length, so no workgroup barrier
// may couple two of them.  Behaviour r of the round owns block r (64 columns of S::words words, the arena's strided-64 layout: lane l
// owns column l, every row access of the wavefront is coalesced) of three buffers: the candidate set K_i lives in set[i & 1], column c
// = its c-th member; `stage` is where lane l builds the successor it is looking at.  In LDS: the observation row, the mask, and the
// fingerprints of the members the next set has so far (64 x 8 B) — 2 * words + 64 words of 8 bytes, dynamic.
// Per observation: every lane that has a candidate loads it; the slot loop runs to the wavefront's largest nslots (as k_simulate's);
// an enabled successor is built into the lane's staging column — with a full mask only when its fingerprint is the observation's — and
// compared under the mask; the lanes that match drop what the next set already holds (fingerprint list first, rows where fingerprints
// agree), then what a lower lane of the same round brings, and the rest is appended by ballot + popcount prefix.  An append past 64
// makes the behaviour AMBIGUOUS (the step's counters are still completed: they are a function of the behaviour alone).
// K_0: the lanes stride over k < num_init.  A launch advances a behaviour by at most `iters` observations; the carry between launches
// is one word per behaviour (behaviour.h beh_carry), the verdict record accumulates in place.  Totals: one atomic of each kind per
// wavefront and launch.
// With unlogged steps (MC_BEH_F_HIDDEN) the host launches k_behaviours<S, 0, true>: the closure of the current set under hidden steps
// fills the lanes behind it (see above the kernel).  The plain instantiation compiles none of that.
#ifndef TLAMC_ENGINE_BEHAVIOURS_H
#define TLAMC_ENGINE_BEHAVIOURS_H

#include "behaviour.h"

namespace mc {

struct BehCounters {
    unsigned long long accepted, rejected, ambiguous, observations, generated;
    unsigned long long first_rejected;   // least index of a rejected behaviour, ~0 = none
};

struct BehArgs {
    uint64_t b0, n;                 // behaviours b0 .. b0+n-1 of the batch are the round's 0 .. n-1
    const uint64_t *first;          // [n + 1]: offsets of the round's behaviours into rows, in observations
    const uint64_t *rows;           // the round's observations, plain rows of S::words words
    const uint64_t *mask;           // S::words words, or NULL: everything is observed
    uint64_t *set0, *set1, *stage;  // n blocks of 64 columns each
    uint64_t *carry;                // [n]
    mc_beh_verdict *out;            // [n]
    BehCounters *ctr;
    uint32_t flags, iters;
};

// the wavefront's append: every lane calls it, `mine` = this lane's staging column holds a matching row of fingerprint fp.  nnext: the
// members the next set holds (uniform), s_fp their fingerprints.  Returns false once the set would pass 64 members.
__device__ __forceinline__ bool beh_append(int W, bool mine, uint64_t fp, const uint64_t *stage_blk, uint64_t *next_blk, uint64_t *s_fp, unsigned &nnext, unsigned mutant) {
    const unsigned lane = threadIdx.x & 63;
    if (!__ballot(mine)) return true;
    // (a lane compares its row with the staging columns of lower lanes: what they built is visible from here on)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const CWordRef my{stage_blk + lane, 64};
    // the members the set already holds
    if (mine && mutant != 4)
        for (unsigned j = 0; j < nnext; ++j)
            if (s_fp[j] == fp && beh_same_row(my, CWordRef{next_blk + j, 64}, W)) { mine = false; break; }
    // ... and what a lower lane of this round brings
    unsigned long long bal = __ballot(mine);
    for (unsigned long long rest = mutant == 1 ? 0ull : bal; rest; rest &= rest - 1) {
        const unsigned j = (unsigned)__builtin_ctzll(rest);
        const uint64_t fj = (uint64_t)__shfl((unsigned long long)fp, (int)j);
        if (mine && lane > j && fj == fp && beh_same_row(my, CWordRef{stage_blk + j, 64}, W)) mine = false;
    }
    bal = __ballot(mine);
    const unsigned pos = nnext + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
    if (mine && pos < MC_BEH_MAX_CANDIDATES) {
        const WordRef dst{next_blk + pos, 64};
        for (int w = 0; w < W; ++w) dst.set(w, my.get(w));
        s_fp[pos] = fp;
    }
    const unsigned total = nnext + (unsigned)__popcll(bal);
    nnext = total < MC_BEH_MAX_CANDIDATES ? total : MC_BEH_MAX_CANDIDATES;
    // the rows and fingerprints just written are read by other lanes of this wavefront in the next append
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    return total <= MC_BEH_MAX_CANDIDATES || mutant == 3;
}

// MUTANT: 0 in the product.  tests/_behshim/behshim.hip also builds 1 (no dedup across the lanes of one round), 2 (the last word of the
// mask skipped) and 3 (lane 64 and beyond dropped in place of AMBIGUOUS): kernels that the device tests must tell from this one.
// tests/_behshim/behgap.hip builds the HIDDEN kernel at 4 (no dedup of the closure against the current set), 5 (the depth bound off by
// one) and 6 (the match against the observation before skipped); each stays inside its 64 columns and its H (+ 1) depths.
//
// HIDDEN: the instantiation for MC_BEH_F_HIDDEN(H) (behaviour.h: unlogged steps).  The closure C of K_{i-1} is appended to the current
// set's own block, behind K_{i-1}; a depth's frontier is the column range [lo, hi) and lane l takes column lo + l; every lane calls
// beh_append twice per slot from the same staging column, towards C (only below depth H, when the successor still matches o_{i-1}) and
// towards K_i.  The rows one lane appends to C and another loads in the next depth are ordered by beh_append's closing fence +
// wave_barrier.  LDS: beh_lds_words(W, true) — o_{i-1} and the fingerprints of C on top of the plain kernel's.  HIDDEN = false
// compiles none of it: the kernel DESIGN section 23 measured.
__host__ __device__ constexpr size_t beh_lds_words(int W, bool hidden) { return (size_t)2 * W + MC_BEH_MAX_CANDIDATES + (hidden ? (size_t)W + MC_BEH_MAX_CANDIDATES : 0); }

template <class S, unsigned MUTANT = 0, bool HIDDEN = false>
__global__ void __launch_bounds__(64)
k_behaviours(typename S::Params prm, BehArgs a) {
    extern __shared__ uint64_t beh_lds[];
    const uint64_t r = blockIdx.x;
    if (r >= a.n) return;
    const unsigned lane = threadIdx.x;
    const int W = S::words(prm);
    uint64_t *s_obs = beh_lds, *s_mask = beh_lds + W, *s_fp = beh_lds + 2 * W;
    const uint64_t o0 = a.first[r], T = a.first[r + 1] - o0;
    uint64_t carry = a.carry[r];
    uint32_t step = beh_carry_step(carry);
    unsigned ncur = beh_carry_n(carry), verdict = beh_carry_verdict(carry);
    if (verdict != BEH_RUNNING) return;   // (uniform: one behaviour, one wavefront)
    const bool full = a.mask == nullptr;
    const int WM = MUTANT == 2 ? W - 1 : W;   // the words a match looks at
    for (int w = lane; w < W; w += 64) s_mask[w] = full ? ~0ull : a.mask[w];
    uint64_t *const stage_blk = a.stage + r * (uint64_t)W * 64;
    const WordRef stage{stage_blk + lane, 64};
    const CWordRef cstage{stage_blk + lane, 64};
    unsigned gen = 0, outside = 0, errors = 0, cand = 0, peak = 0, nobs = 0;
    for (uint32_t it = 0; it < a.iters && step < T; ++it) {
        for (int w = lane; w < W; w += 64) s_obs[w] = a.rows[(o0 + step) * W + w];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const uint64_t ofp = full ? S::fp_of(prm, CWordRef{s_obs, 1}) : 0;
        uint64_t *const cur_blk = ((step + 1) & 1 ? a.set1 : a.set0) + r * (uint64_t)W * 64;
        uint64_t *const next_blk = (step & 1 ? a.set1 : a.set0) + r * (uint64_t)W * 64;
        unsigned nnext = 0;
        bool fits = true;
        ++nobs;
        if (step == 0) {
            const uint64_t ni = S::num_init(prm);
            for (uint64_t k0 = 0; k0 < ni; k0 += 64) {
                const uint64_t k = k0 + lane;
                bool mine = false;
                uint64_t fp = 0;
                if (k < ni) {
                    S::init(prm, k, stage);
                    ++gen;
                    if (beh_match(cstage, s_obs, s_mask, WM)) {
                        mine = true;
                        if (S::init_status(prm, cstage) & ST_OUT_OF_MODEL) ++outside;
                        fp = S::fp_of(prm, cstage);
                    }
                }
                fits = beh_append(W, mine, fp, stage_blk, next_blk, s_fp, nnext, MUTANT) && fits;
            }
        } else if constexpr (HIDDEN) {
            uint64_t *const s_prev = beh_lds + 2 * W + MC_BEH_MAX_CANDIDATES, *const s_cfp = s_prev + W;
            const unsigned H = beh_hidden(a.flags), HD = MUTANT == 5 ? H + 1 : H;   // the depth below which a successor may join C
            for (int w = lane; w < W; w += 64) s_prev[w] = a.rows[(o0 + step - 1) * W + w];
            if (lane < ncur) s_cfp[lane] = S::fp_of(prm, CWordRef{cur_blk + lane, 64});
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
            const uint64_t pfp = full ? S::fp_of(prm, CWordRef{s_prev, 1}) : 0;
            unsigned nclo = ncur, lo = 0;
            bool cfits = true;
            for (unsigned d = 0; d <= HD && cfits && lo < nclo; ++d) {   // (at d == HD nothing joins C: the loop ends there at the latest)
                const unsigned hi = nclo;   // hi - lo <= 64: C never passes 64 columns
                const bool have = lo + lane < hi;
                const CWordRef cur{cur_blk + (have ? lo + lane : 0), 64};
                typename S::Local loc;
                int ns = 0;
                if (have) {
                    S::load(prm, cur, loc);
                    ns = S::nslots(prm, loc);
                }
                if (a.flags & MC_BEH_F_STUTTER) {
                    const bool mine = have && beh_match(cur, s_obs, s_mask, WM);
                    uint64_t fp = 0;
                    if (mine) {
                        for (int w = 0; w < W; ++w) stage.set(w, cur.get(w));
                        fp = s_cfp[lo + lane];
                    }
                    fits = beh_append(W, mine, fp, stage_blk, next_blk, s_fp, nnext, MUTANT < 4 ? MUTANT : 0) && fits;
                }
                const int wns = (int)wave_max_u32((unsigned)ns);
                for (int slot = 0; slot < wns; ++slot) {
                    bool to_next = false, to_clo = false;
                    uint64_t fp = 0;
                    if (have && slot < ns) {
                        uint64_t f = 0;
                        const unsigned st = S::eval(prm, loc, cur, slot, f);
                        const unsigned kind = beh_step_kind(st);
                        if (kind != BEH_NO_STEP) ++gen;
                        if (kind == BEH_ERROR) ++errors;
                        if (kind == BEH_STEP || kind == BEH_STEP_OUTSIDE) {
                            const bool known = beh_fp_known(st);
                            if (!(full && known && f != ofp && f != pfp)) {
                                if (st & ST_SELFLOOP) { for (int w = 0; w < W; ++w) stage.set(w, cur.get(w)); }
                                else S::apply(prm, cur, slot, stage);
                                to_next = beh_match(cstage, s_obs, s_mask, WM);
                                to_clo = d < HD && (MUTANT == 6 || beh_match(cstage, s_prev, s_mask, WM));
                                if (to_next && kind == BEH_STEP_OUTSIDE) ++outside;
                                if (to_next || to_clo) fp = known ? f : S::fp_of(prm, cstage);
                            }
                        }
                    }
                    cfits = beh_append(W, to_clo, fp, stage_blk, cur_blk, s_cfp, nclo, MUTANT == 4 ? 4 : 0) && cfits;
                    fits = beh_append(W, to_next, fp, stage_blk, next_blk, s_fp, nnext, MUTANT < 4 ? MUTANT : 0) && fits;
                }
                lo = hi;
            }
            if (!cfits) fits = false;
            if (fits) peak = peak > nclo ? peak : nclo;
        } else {
            const bool have = lane < ncur;
            const CWordRef cur{cur_blk + lane, 64};
            typename S::Local loc;
            int ns = 0;
            if (have) {
                S::load(prm, cur, loc);
                ns = S::nslots(prm, loc);
            }
            if (a.flags & MC_BEH_F_STUTTER) {
                const bool mine = have && beh_match(cur, s_obs, s_mask, WM);
                uint64_t fp = 0;
                if (mine) {
                    for (int w = 0; w < W; ++w) stage.set(w, cur.get(w));
                    fp = S::fp_of(prm, cur);
                }
                fits = beh_append(W, mine, fp, stage_blk, next_blk, s_fp, nnext, MUTANT) && fits;
            }
            const int wns = (int)wave_max_u32((unsigned)ns);
            for (int slot = 0; slot < wns; ++slot) {
                bool mine = false;
                uint64_t fp = 0;
                if (have && slot < ns) {
                    uint64_t f = 0;
                    const unsigned st = S::eval(prm, loc, cur, slot, f);
                    const unsigned kind = beh_step_kind(st);
                    if (kind != BEH_NO_STEP) ++gen;
                    if (kind == BEH_ERROR) ++errors;
                    if (kind == BEH_STEP || kind == BEH_STEP_OUTSIDE) {
                        const bool known = beh_fp_known(st);
                        if (!(full && known && f != ofp)) {
                            if (st & ST_SELFLOOP) { for (int w = 0; w < W; ++w) stage.set(w, cur.get(w)); }
                            else S::apply(prm, cur, slot, stage);
                            if (beh_match(cstage, s_obs, s_mask, WM)) {
                                mine = true;
                                if (kind == BEH_STEP_OUTSIDE) ++outside;
                                fp = known ? f : S::fp_of(prm, cstage);
                            }
                        }
                    }
                }
                fits = beh_append(W, mine, fp, stage_blk, next_blk, s_fp, nnext, MUTANT) && fits;
            }
        }
        if (!fits) { verdict = MC_BEH_AMBIGUOUS; break; }
        if (nnext == 0) { verdict = MC_BEH_REJECTED; break; }
        ncur = cand = nnext;
        peak = peak > nnext ? peak : nnext;
        ++step;
    }
    if (verdict == BEH_RUNNING && step >= T) verdict = MC_BEH_ACCEPTED;
    const unsigned gsum = wave_sum_u32(gen), osum = wave_sum_u32(outside), esum = wave_sum_u32(errors);
    if (lane == 0) {
        a.carry[r] = beh_carry(step, ncur, verdict);
        mc_beh_verdict v = a.out[r];
        v.verdict = (int32_t)verdict;
        v.step = step;
        if (cand) v.candidates = cand;
        v.peak = v.peak > peak ? v.peak : peak;
        v.generated += gsum;
        v.outside += osum;
        v.errors += esum;
        a.out[r] = v;
        if (gsum) atomicAdd(&a.ctr->generated, (unsigned long long)gsum);
        if (nobs) atomicAdd(&a.ctr->observations, (unsigned long long)nobs);
        if (verdict == MC_BEH_ACCEPTED) atomicAdd(&a.ctr->accepted, 1ull);
        if (verdict == MC_BEH_AMBIGUOUS) atomicAdd(&a.ctr->ambiguous, 1ull);
        if (verdict == MC_BEH_REJECTED) {
            atomicAdd(&a.ctr->rejected, 1ull);
            atomicMin(&a.ctr->first_rejected, (unsigned long long)(a.b0 + r));
        }
    }
}

}  // namespace mc

#endif  // TLAMC_ENGINE_BEHAVIOURS_H
