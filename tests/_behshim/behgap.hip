// tests/_behshim/behgap.hip — TEST-ONLY driver of k_behaviours<S, MUTANT, true> (tla_rust_amd/csrc/engine_behaviours.h: the
// instantiation for unlogged steps, MC_BEH_F_HIDDEN) over the lowering SpecGap (behgap.h), built four times: -DBEH_MUTANT=0 is the
// product's kernel, 4 / 5 / 6 are the kernel with one thing broken (no dedup of the closure against the current set; the depth bound
// off by one; the match against the observation before skipped).  tests/test_gpu_behaviours_hidden.py runs the same cases on all four
// and on the host rule (beh_check over the same lowering, compiled into this library too): the product's kernel must give the host's
// verdicts, each mutant must not on the case made for it.  A library of its own: nothing of libtlamc.so is linked.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "behgap.h"
#include "hip_owned.h"
#include "engine_kernels.h"
#include "engine_behaviours.h"

#ifndef BEH_MUTANT
#define BEH_MUTANT 0
#endif

static std::string g_error;
extern "C" void mc_set_error_internal(const char *msg) { g_error = msg ? msg : ""; }
extern "C" const char *bg_last_error() { return g_error.c_str(); }
extern "C" int bg_mutant() { return BEH_MUTANT; }

using namespace mc;

extern "C" int bg_host(uint64_t K, uint64_t h0, int G, int B, int on, uint64_t count, const uint64_t *first, const uint64_t *rows, const uint64_t *mask,
                       unsigned flags, mc_beh_verdict *out) {
    return gap_host(SpecGap::Params{K, h0, G, B, on, 0}, count, first, rows, mask, flags, out);
}

// the kernel (this build's MUTANT), launched as engine.hip launches it: one round, ceil(longest / iters) launches
extern "C" int bg_device(uint64_t K, uint64_t h0, int G, int B, int on, uint64_t count, const uint64_t *first, const uint64_t *rows, const uint64_t *mask,
                         unsigned flags, uint32_t iters, mc_beh_verdict *out) {
    const SpecGap::Params prm{K, h0, G, B, on, 0};
    const int W = 2;
    if (!count || !iters || K > MC_BEH_MAX_INIT || B < 0 || B > 64) return MC_EBADCFG;
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
    const size_t lds = beh_lds_words(W, true) * sizeof(uint64_t);
    for (uint64_t l = 0; l < (longest + iters - 1) / iters; ++l) {
        hipLaunchKernelGGL((k_behaviours<SpecGap, BEH_MUTANT, true>), dim3((unsigned)count), dim3(64), lds, 0, prm, a);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out, count * sizeof(mc_beh_verdict), hipMemcpyDeviceToHost));
    return MC_OK;
}
