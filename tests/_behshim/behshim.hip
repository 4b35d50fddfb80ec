// tests/_behshim/behshim.hip — TEST-ONLY driver of k_behaviours (tla_rust_amd/csrc/engine_behaviours.h) over a lowering written for
// it, built four times: -DBEH_MUTANT=0 is the product's kernel, 1 / 2 / 3 are the kernel with one thing broken (no dedup across the
// lanes of one round; the last word of the mask skipped; lane 64 and beyond dropped in place of AMBIGUOUS).  tests/test_gpu_behaviours.py
// runs the same cases on all four and on the host rule (beh_check of behaviour.h over the same lowering, compiled into this library
// too): the product's kernel must give the host's verdicts, each mutant must not.  A library of its own: nothing of libtlamc.so is
// linked; the product's headers are included unchanged.
//
// SpecHide: a row is two words, x (logged) and h (hidden, or logged through the LAST word of the mask).  num_init = K initial states
// (x = 0, h = k).  Slot 0: x' = x + 1, h' = h / 2 — rows 2j and 2j + 1 have one successor, and as members 2j and 2j + 1 of a set they
// sit in neighbouring lanes and bring it in the same round.  Slots 1 .. B: x' = x + 1, h' = h * B + slot - 1 + 1000 — B fresh rows per
// member: a set that grows past 64.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "spec_registry.h"
#include "hip_owned.h"
#include "engine_kernels.h"
#include "engine_behaviours.h"

#ifndef BEH_MUTANT
#define BEH_MUTANT 0
#endif

static std::string g_error;
extern "C" void mc_set_error_internal(const char *msg) { g_error = msg ? msg : ""; }
extern "C" const char *bd_last_error() { return g_error.c_str(); }
extern "C" int bd_mutant() { return BEH_MUTANT; }

namespace mc {
struct SpecHide {
    struct Params { uint64_t K; int B; int pad; };
    struct Local { uint64_t x, h; };
    static constexpr int MAX_WORDS = 2;
    MC_HD static int words(const Params &) { return 2; }
    MC_HD static uint64_t num_init(const Params &p) { return p.K; }
    MC_HD static void init(const Params &, uint64_t k, WordRef out) { out.set(0, 0); out.set(1, k); }
    MC_HD static unsigned init_status(const Params &, CWordRef) { return ST_ENABLED; }
    MC_HD static uint64_t fp2(uint64_t x, uint64_t h) { return fp_nonzero(fmix64(x * 0x9e3779b97f4a7c15ull ^ fmix64(h + 1))); }
    MC_HD static uint64_t fp_of(const Params &, CWordRef s) { return fp2(s.get(0), s.get(1)); }
    MC_HD static void load(const Params &, CWordRef s, Local &l) { l.x = s.get(0); l.h = s.get(1); }
    MC_HD static int nslots(const Params &p, const Local &) { return 1 + p.B; }
    MC_HD static uint64_t next_h(const Params &p, uint64_t h, int slot) { return slot == 0 ? h / 2 : h * (uint64_t)p.B + (uint64_t)slot + 999; }
    MC_HD static unsigned eval(const Params &p, const Local &l, CWordRef, int slot, uint64_t &fp) {
        if (slot < 0 || slot > p.B || l.x >= 8) return 0;
        fp = fp2(l.x + 1, next_h(p, l.h, slot));
        return ST_ENABLED;
    }
    MC_HD static unsigned apply(const Params &p, CWordRef s, int slot, WordRef out) {
        const uint64_t x = s.get(0), h = s.get(1);
        out.set(0, x + 1);
        out.set(1, next_h(p, h, slot));
        return ST_ENABLED;
    }
};
}  // namespace mc

using namespace mc;

// the host rule over SpecHide
extern "C" int bd_host(uint64_t K, int B, uint64_t count, const uint64_t *first, const uint64_t *rows, const uint64_t *mask, unsigned flags,
                       mc_beh_verdict *out) {
    const SpecHide::Params prm{K, B, 0};
    for (uint64_t b = 0; b < count; ++b)
        if (int rc = beh_check<SpecHide>(prm, rows + first[b] * 2, first[b + 1] - first[b], mask, flags, &out[b], nullptr)) return rc;
    return MC_OK;
}

// the kernel (this build's MUTANT), launched as engine.hip launches it: one round, ceil(longest / iters) launches
extern "C" int bd_device(uint64_t K, int B, uint64_t count, const uint64_t *first, const uint64_t *rows, const uint64_t *mask, unsigned flags,
                         uint32_t iters, mc_beh_verdict *out) {
    const SpecHide::Params prm{K, B, 0};
    const int W = 2;
    if (!count || !iters || K > MC_BEH_MAX_INIT) return MC_EBADCFG;
    uint64_t longest = 0;
    for (uint64_t b = 0; b < count; ++b) {
        if (first[b + 1] <= first[b]) return MC_EBADCFG;
        longest = std::max(longest, first[b + 1] - first[b]);
    }
    const uint64_t nrows = first[count];
    DevBuf<uint64_t> set0, set1, stage, d_rows, d_first, carry, d_mask;
    DevBuf<mc_beh_verdict> d_out;
    DevBuf<BehCounters> ctr;
    HIP_TRY(set0.alloc(count * 64 * W));
    HIP_TRY(set1.alloc(count * 64 * W));
    HIP_TRY(stage.alloc(count * 64 * W));
    HIP_TRY(d_rows.alloc(nrows * W));
    HIP_TRY(d_first.alloc(count + 1));
    HIP_TRY(carry.alloc(count));
    HIP_TRY(d_out.alloc(count));
    HIP_TRY(ctr.alloc(1));
    HIP_TRY(hipMemcpy(d_rows, rows, nrows * W * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_first, first, (count + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(carry, 0, count * sizeof(uint64_t)));
    HIP_TRY(hipMemset(d_out, 0, count * sizeof(mc_beh_verdict)));
    BehCounters c{};
    c.first_rejected = ~0ull;
    HIP_TRY(hipMemcpy(ctr, &c, sizeof c, hipMemcpyHostToDevice));
    const bool full = beh_mask_full(mask, W);
    if (!full) {
        HIP_TRY(d_mask.alloc(W));
        HIP_TRY(hipMemcpy(d_mask, mask, W * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    BehArgs a{};
    a.b0 = 0;
    a.n = count;
    a.first = d_first;
    a.rows = d_rows;
    a.mask = full ? nullptr : (const uint64_t *)d_mask;
    a.set0 = set0;
    a.set1 = set1;
    a.stage = stage;
    a.carry = carry;
    a.out = d_out;
    a.ctr = ctr;
    a.flags = flags;
    a.iters = iters;
    const size_t lds = ((size_t)2 * W + MC_BEH_MAX_CANDIDATES) * sizeof(uint64_t);
    for (uint64_t l = 0; l < (longest + iters - 1) / iters; ++l) {
        hipLaunchKernelGGL((k_behaviours<SpecHide, BEH_MUTANT>), dim3((unsigned)count), dim3(64), lds, 0, prm, a);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out, count * sizeof(mc_beh_verdict), hipMemcpyDeviceToHost));
    return MC_OK;
}
