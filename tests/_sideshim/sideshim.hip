// sideshim.hip — a test-only driver of the passes that run after or beside the search and are templated on a lowering S:
// engine_graph.h (k_graph_index, k_graph_degree, k_graph_fill, k_live_proc, k_live_unit, k_live_pred), engine_coverage.h
// (k_coverage_generated, k_coverage_distinct) and engine_violations.h (k_viol_stored, k_viol_frontier), instantiated with the table
// lowering of spec_table.h on rows that no search produced (tests/sideshim.py, tests/sidemodel.py).  A library of its own: nothing of
// libtlamc.so is linked.  The product's headers are included unchanged, in engine.hip's order (the two it has in between,
// engine_pairs.h and engine_sim.h, hold no pass driven here), and every kernel is launched with the grid, the block and the chunks
// engine.hip gives it: each_chunk is the product's (engine_coverage.h), the plain chunks of viol_stored / cov_distinct are restated.
// The exclusive scan between the degree and the fill pass is a HOST cumulative sum, for the reason tests/_xchgshim/xchgshim.hip gives:
// the product's scans are non-inline functions of the translation unit that holds the state-graph passes and their host half.
// Rows arrive in the LOGICAL layout (state-major, S::words words each) and are blocked here as the arena holds them (arena_cref: 64
// states per block, word-major).  Every buffer a kernel writes lies between two guard zones of GUARD elements filled with CANARY bytes;
// what the caller hands in as an output is uploaded as it is, so its pre-fill comes back wherever the kernel wrote nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <type_traits>
#include <string>
#include <vector>

#include "spec_registry.h"
#include "hip_owned.h"
#include "engine_kernels.h"
#include "engine_coverage.h"
#include "engine_violations.h"
#include "engine_graph.h"
#include "spec_table.h"

static std::string g_error;
extern "C" void mc_set_error_internal(const char *msg) { g_error = msg ? msg : ""; }
extern "C" const char *sd_last_error() { return g_error.c_str(); }

namespace {
using namespace mc;

constexpr uint64_t GUARD = 64;
constexpr int CANARY = 0xc5;

int bad(const char *what) { set_error(std::string("sideshim: ") + what); return MC_EBADCFG; }

// `count` elements between two guard zones
template <class T>
struct Guarded {
    DevBuf<T> buf;
    uint64_t count = 0;
    T *p() const { return buf.p + GUARD; }
    int make(const T *src, uint64_t n) {
        count = n;
        HIP_TRY(buf.alloc(n + 2 * GUARD));
        HIP_TRY(hipMemset(buf.p, CANARY, (n + 2 * GUARD) * sizeof(T)));
        if (n) HIP_TRY(hipMemcpy(p(), src, n * sizeof(T), hipMemcpyHostToDevice));
        return MC_OK;
    }
    int fill(int byte) {
        if (count) HIP_TRY(hipMemset(p(), byte, count * sizeof(T)));
        return MC_OK;
    }
    int fetch(T *dst) const {
        if (count) HIP_TRY(hipMemcpy(dst, p(), count * sizeof(T), hipMemcpyDeviceToHost));
        return MC_OK;
    }
    // clears *intact when a byte of either guard zone changed
    int check(int *intact) const {
        std::vector<unsigned char> h(GUARD * sizeof(T));
        for (int side = 0; side < 2; ++side) {
            HIP_TRY(hipMemcpy(h.data(), side ? (const void *)(p() + count) : (const void *)buf.p, h.size(), hipMemcpyDeviceToHost));
            for (unsigned char c : h) if (c != CANARY) *intact = 0;
        }
        return MC_OK;
    }
};

int finish() {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return MC_OK;
}

int params_ok(const SpecTabParams &p, uint64_t chunk) {
    if (p.max_slots < 1 || p.max_slots > SPECTAB_MAX_SLOTS) return bad("max_slots: 1 .. 64");
    if (p.nbins < 1 || p.nbins > COV_MAX_BINS) return bad("nbins: 1 .. COV_MAX_BINS");
    if (p.ninst < 0 || p.ninst > 8 || p.maxch < 1) return bad("ninst: 0 .. 8, maxch >= 1");
    if (chunk < 64 || chunk % 64) return bad("chunk: a multiple of 64, at least 64");
    return MC_OK;
}

// the rows as the arena holds them: whole 64-state blocks, word-major (arena_cref)
int upload_arena(const SpecTabParams &prm, const uint64_t *rows, uint64_t n, DevBuf<uint64_t> &arena) {
    const uint64_t W = (uint64_t)SpecTab::words(prm), blocks = (n + 63) / 64 + 1;   // (one block of slack: zero rows)
    std::vector<uint64_t> h(blocks * W * 64, 0);
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t w = 0; w < W; ++w) h[((i >> 6) * W) * 64 + w * 64 + (i & 63)] = rows[i * W + w];
    HIP_TRY(arena.alloc(h.size()));
    HIP_TRY(hipMemcpy(arena.p, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    return MC_OK;
}

// trace records: a parent is none (0xffffffff) or the index of a row that exists; a slot lies inside the row
int records_ok(const SpecTabParams &prm, const uint32_t *parent, const uint16_t *pslot, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        if (parent[i] != 0xffffffffu && parent[i] >= n) return bad("a parent index beyond the rows");
        if ((int)pslot[i] >= prm.max_slots) return bad("a parent slot beyond the row");
    }
    return MC_OK;
}

template <class T>
int upload(DevBuf<T> &d, const T *src, uint64_t n) {
    HIP_TRY(d.alloc(n ? n : 1));
    if (n) HIP_TRY(hipMemcpy(d.p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return MC_OK;
}

void counters_out(const GraphCounters &gc, uint64_t *out) {
    out[0] = gc.missing_states; out[1] = gc.missing_succ; out[2] = gc.first_bad; out[3] = gc.dropped; out[4] = gc.self_loops; out[5] = gc.max_degree;
}

template <class S>
int violations(const SpecTabParams &prm, const uint64_t *arena, const uint32_t *parent, const uint16_t *pslot, uint64_t lo, uint64_t hi, uint64_t new_hi,
               int expanded, unsigned flags, uint64_t chunk, ViolBins *bins) {
    // Engine::viol_stored: plain chunks
    auto stored = [&](uint64_t a, uint64_t b) {
        for (uint64_t c0 = a; c0 < b; c0 += chunk) {
            const uint64_t c1 = c0 + chunk < b ? c0 + chunk : b;
            hipLaunchKernelGGL(k_viol_stored<S>, dim3((unsigned)((c1 - c0 + 255) / 256)), dim3(256), 0, 0, prm, arena, parent, pslot, c0, c1, bins);
        }
    };
    // Engine::viol_level
    if (expanded)
        each_chunk(lo, hi, chunk, [&](uint64_t c0, uint64_t c1, uint64_t ncols) {
            hipLaunchKernelGGL(k_viol_frontier<S>, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, 0, prm, arena, c0, c1, ncols, flags, bins);
        });
    if (!expanded || ChecksOnExpand<S>::value) stored(lo, hi);
    else stored(hi, new_hi);
    return finish();
}

}  // namespace

extern "C" {

unsigned sd_guard() { return (unsigned)GUARD; }
unsigned sd_cov_max_bins() { return COV_MAX_BINS; }
unsigned sd_viol_bins() { return VIOL_BINS; }
unsigned sd_sparse_slots() { return MC_SPARSE_SLOTS; }

// Engine::graph_build's sequence over rows[n] (the first `expanded` of them have out-edges) and a seen-set of nbuckets buckets in the
// 8-slot or the sparse form, then k_live_proc, k_live_unit (unit_tab[ninst * nlabels]) and k_live_pred (npred predicates) in the
// engine's chunks.  slot_index (one entry per table slot), degree and offsets (n + 1), pred (n): written whole, the first three after
// the memsets graph_build does, pred after predicates_build's.  dst, act, proc, unit: cap elements each, handed in pre-filled and handed
// back; cap must hold the edges the degree pass counts.  gc_degree / gc_fill: missing_states, missing_succ, first_bad, dropped,
// self_loops, max_degree after each pass (the fill pass adds to the degree pass's).  The fill pass runs whatever the degree pass found:
// its writes lie inside offsets[] either way.
int sd_graph(const SpecTabParams *prm_, const uint64_t *rows, uint64_t n, uint64_t expanded, const uint64_t *table, uint64_t nbuckets, int sparse,
             uint64_t chunk, const int8_t *unit_tab, int nlabels, int npred, uint64_t cap, uint32_t *slot_index, uint32_t *degree, uint64_t *offsets,
             uint32_t *dst, int16_t *act, int8_t *proc, int8_t *unit, uint32_t *pred, uint64_t *gc_degree, uint64_t *gc_fill, uint64_t *pred_bad,
             uint64_t *edges_out, int *intact) {
    const SpecTabParams prm = *prm_;
    if (int rc = params_ok(prm, chunk)) return rc;
    if (!n || expanded > n || n + 1 > 0x7fffffffull || !nbuckets) return bad("graph: 1 .. 2^31 - 2 rows, expanded <= rows, a table");
    if (nlabels < 1 || npred < 0 || npred > LIVE_MAX_PREDS) return bad("graph: nlabels >= 1, at most 32 predicates");
    HIP_TRY(hipSetDevice(0));
    using S = SpecTab;
    const uint64_t table_cap = nbuckets * (uint64_t)(sparse ? MC_SPARSE_SLOTS : 8);
    const uint64_t seen = sparse ? (nbuckets | SEEN_SPARSE) : nbuckets;
    DevBuf<uint64_t> d_arena, d_table;
    DevBuf<int8_t> d_unit_tab;
    Guarded<uint32_t> g_index, g_degree, g_dst, g_pred;
    Guarded<uint64_t> g_off;
    Guarded<int16_t> g_act;
    Guarded<int8_t> g_proc, g_unit;
    Guarded<GraphCounters> g_gc;
    Guarded<unsigned long long> g_bad;
    if (int rc = upload_arena(prm, rows, n, d_arena)) return rc;
    if (int rc = upload(d_table, table, table_cap)) return rc;
    if (int rc = upload(d_unit_tab, unit_tab, (uint64_t)(prm.ninst > 0 ? prm.ninst : 1) * (uint64_t)nlabels)) return rc;
    GraphCounters gc;
    memset(&gc, 0, sizeof gc);
    gc.first_bad = ~0ull;
    unsigned long long pbad = ~0ull;
    if (int rc = g_gc.make(&gc, 1)) return rc;
    if (int rc = g_bad.make(&pbad, 1)) return rc;
    if (int rc = g_index.make(slot_index, table_cap)) return rc;
    if (int rc = g_degree.make(degree, n + 1)) return rc;
    if (int rc = g_off.make(offsets, n + 1)) return rc;
    if (int rc = g_pred.make(pred, n)) return rc;
    if (int rc = g_dst.make(dst, cap)) return rc;
    if (int rc = g_act.make(act, cap)) return rc;
    if (int rc = g_proc.make(proc, cap)) return rc;
    if (int rc = g_unit.make(unit, cap)) return rc;
    const uint64_t *arena = d_arena.p, *tab = d_table.p;
    auto chunks = [&](auto kernel, uint64_t lo, uint64_t hi, auto... args) {   // Engine::graph_chunks
        each_chunk(lo, hi, chunk, [&](uint64_t c0, uint64_t c1, uint64_t ncols) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, 0, prm, arena, c0, c1, ncols, tab, seen, args...);
        });
    };
    // Engine::graph_build
    if (int rc = g_index.fill(0xff)) return rc;
    if (int rc = g_degree.fill(0)) return rc;
    hipLaunchKernelGGL(k_graph_index<S>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, prm, arena, n, tab, seen, g_index.p(), table_cap, g_gc.p());
    chunks(k_graph_degree<S>, 0, expanded, g_degree.p(), g_gc.p());
    if (int rc = finish()) return rc;
    if (int rc = g_degree.fetch(degree)) return rc;
    uint64_t run = 0;
    for (uint64_t i = 0; i <= n; ++i) { offsets[i] = run; run += degree[i]; }
    const uint64_t edges = offsets[n];
    *edges_out = edges;
    if (int rc = g_gc.fetch(&gc)) return rc;
    counters_out(gc, gc_degree);
    if (edges > cap) return bad("graph: the degree pass counted more edges than the outputs hold");
    HIP_TRY(hipMemcpy(g_off.p(), offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    chunks(k_graph_fill<S>, 0, expanded, (const uint32_t *)g_index.p(), table_cap, (const uint64_t *)g_off.p(), g_dst.p(), g_act.p(), g_gc.p());
    if (int rc = finish()) return rc;
    if (int rc = g_gc.fetch(&gc)) return rc;
    counters_out(gc, gc_fill);
    // Engine::liveness / liveness_units / predicates_build
    chunks(k_live_proc<S>, 0, expanded, (const uint64_t *)g_off.p(), g_proc.p());
    chunks(k_live_unit<S>, 0, expanded, (const uint64_t *)g_off.p(), LiveUnitTab{prm.ninst, nlabels, (const int8_t *)d_unit_tab.p}, g_unit.p());
    LivePredTab ptab;
    memset(&ptab, 0, sizeof ptab);
    ptab.n = npred;
    if (int rc = g_pred.fill(0)) return rc;
    if (ptab.n) chunks(k_live_pred<S>, 0, n, ptab, g_pred.p(), g_bad.p());
    if (int rc = finish()) return rc;
    if (int rc = g_index.fetch(slot_index)) return rc;
    if (int rc = g_dst.fetch(dst)) return rc;
    if (int rc = g_act.fetch(act)) return rc;
    if (int rc = g_proc.fetch(proc)) return rc;
    if (int rc = g_unit.fetch(unit)) return rc;
    if (int rc = g_pred.fetch(pred)) return rc;
    if (int rc = g_bad.fetch(&pbad)) return rc;
    *pred_bad = pbad;
    *intact = 1;
    if (int rc = g_gc.check(intact)) return rc;
    if (int rc = g_bad.check(intact)) return rc;
    if (int rc = g_index.check(intact)) return rc;
    if (int rc = g_degree.check(intact)) return rc;
    if (int rc = g_off.check(intact)) return rc;
    if (int rc = g_pred.check(intact)) return rc;
    if (int rc = g_dst.check(intact)) return rc;
    if (int rc = g_act.check(intact)) return rc;
    if (int rc = g_proc.check(intact)) return rc;
    return g_unit.check(intact);
}

// Engine::cov_generated over [gen_lo, gen_hi) and Engine::cov_distinct over [dist_lo, dist_hi) of rows[n] with the trace records
// parent / pslot [n].  bins: 2 * prm.nbins counters (generated, then distinct), handed in with whatever they hold and handed back.
int sd_coverage(const SpecTabParams *prm_, const uint64_t *rows, uint64_t n, const uint32_t *parent, const uint16_t *pslot, uint64_t gen_lo, uint64_t gen_hi,
                uint64_t dist_lo, uint64_t dist_hi, uint64_t chunk, uint64_t *bins, int *intact) {
    const SpecTabParams prm = *prm_;
    if (int rc = params_ok(prm, chunk)) return rc;
    if (!n || gen_lo > gen_hi || gen_hi > n || dist_lo > dist_hi || dist_hi > n) return bad("coverage: the ranges must lie inside the rows");
    if (int rc = records_ok(prm, parent, pslot, n)) return rc;
    HIP_TRY(hipSetDevice(0));
    using S = SpecTab;
    DevBuf<uint64_t> d_arena;
    DevBuf<uint32_t> d_parent;
    DevBuf<uint16_t> d_pslot;
    Guarded<unsigned long long> g_bins;
    if (int rc = upload_arena(prm, rows, n, d_arena)) return rc;
    if (int rc = upload(d_parent, parent, n)) return rc;
    if (int rc = upload(d_pslot, pslot, n)) return rc;
    if (int rc = g_bins.make((const unsigned long long *)bins, 2 * (uint64_t)prm.nbins)) return rc;
    const uint64_t *arena = d_arena.p;
    each_chunk(gen_lo, gen_hi, chunk, [&](uint64_t c0, uint64_t c1, uint64_t ncols) {   // Engine::cov_generated
        hipLaunchKernelGGL(k_coverage_generated<S>, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, 0, prm, arena, c0, c1, ncols, g_bins.p(), prm.nbins);
    });
    for (uint64_t c0 = dist_lo; c0 < dist_hi; c0 += chunk) {   // Engine::cov_distinct: plain chunks
        const uint64_t c1 = c0 + chunk < dist_hi ? c0 + chunk : dist_hi;
        hipLaunchKernelGGL(k_coverage_distinct<S>, dim3((unsigned)((c1 - c0 + 255) / 256)), dim3(256), 0, 0, prm, arena, (const uint32_t *)d_parent.p,
                           (const uint16_t *)d_pslot.p, c0, c1, g_bins.p() + prm.nbins, prm.nbins);
    }
    if (int rc = finish()) return rc;
    if (int rc = g_bins.fetch((unsigned long long *)bins)) return rc;
    *intact = 1;
    return g_bins.check(intact);
}

// The passes of Engine::viol_level for the level that expanded [lo, hi) and stored [hi, new_hi) (expanded == 0: only stored states are
// looked at), for SpecTab (stored_variant == 0) or SpecTabStored.  bins: 2 * 2 * VIOL_BINS words, ViolBins as it is (count[], first[]),
// handed in with whatever they hold and handed back.
int sd_violations(int stored_variant, const SpecTabParams *prm_, const uint64_t *rows, uint64_t n, const uint32_t *parent, const uint16_t *pslot, uint64_t lo,
                  uint64_t hi, uint64_t new_hi, int expanded, unsigned flags, uint64_t chunk, uint64_t *bins, int *intact) {
    const SpecTabParams prm = *prm_;
    if (int rc = params_ok(prm, chunk)) return rc;
    if (!n || lo > hi || hi > new_hi || new_hi > n) return bad("violations: lo <= hi <= new_hi <= rows");
    if (int rc = records_ok(prm, parent, pslot, n)) return rc;
    HIP_TRY(hipSetDevice(0));
    static_assert(sizeof(ViolBins) == 2 * VIOL_CELLS * sizeof(uint64_t), "ViolBins is count[] then first[]");
    DevBuf<uint64_t> d_arena;
    DevBuf<uint32_t> d_parent;
    DevBuf<uint16_t> d_pslot;
    Guarded<ViolBins> g_bins;
    if (int rc = upload_arena(prm, rows, n, d_arena)) return rc;
    if (int rc = upload(d_parent, parent, n)) return rc;
    if (int rc = upload(d_pslot, pslot, n)) return rc;
    if (int rc = g_bins.make((const ViolBins *)bins, 1)) return rc;
    const int rc = stored_variant
        ? violations<SpecTabStored>(prm, d_arena.p, d_parent.p, d_pslot.p, lo, hi, new_hi, expanded, flags, chunk, g_bins.p())
        : violations<SpecTab>(prm, d_arena.p, d_parent.p, d_pslot.p, lo, hi, new_hi, expanded, flags, chunk, g_bins.p());
    if (rc) return rc;
    if (int rc2 = g_bins.fetch((ViolBins *)bins)) return rc2;
    *intact = 1;
    return g_bins.check(intact);
}

}  // extern "C"
