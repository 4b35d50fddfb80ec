// xchgshim.hip — a test-only driver of the exchange half of the sharded engine (tla_rust_amd/csrc/engine_kernels.h, "sharded step kernels":
// k_compact_buckets, k_compact_packed, k_gather_range_ends + k_compact_new, k_send_parents, k_ingest, k_ingest_parents, k_bump_arena_next,
// and k_gather_states) on arrays that no search produced (tests/xchgshim.py, tests/xchgmodel.py).  A library of its own: nothing of
// libtlamc.so is linked and no spec template is instantiated.  The product's headers are included unchanged, in engine.hip's order, and
// every kernel is launched with the grid and the block engine.hip gives it.
// The inclusive scan of the answers is a HOST cumulative sum: the product's scan_answers_inclusive (engine_live.h) is a non-inline
// function of the translation unit that also holds the state-graph passes and their host half, so it cannot be linked without them.
// Every buffer a kernel writes (and the scan it reads one behind) lies between two guard zones of GUARD elements filled with CANARY
// bytes; what the caller hands in as an output is uploaded as it is, so its pre-fill comes back wherever the kernel wrote nothing.
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

static std::string g_error;
extern "C" void mc_set_error_internal(const char *msg) { g_error = msg ? msg : ""; }
extern "C" const char *xs_last_error() { return g_error.c_str(); }

namespace {
using namespace mc;

constexpr uint64_t GUARD = 64;
constexpr int CANARY = 0xc5;

int bad(const char *what) { set_error(std::string("xchgshim: ") + what); return MC_EBADCFG; }

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

// a counter block with arena_next set
int fresh_counters(DevBuf<DevCounters> &ctr, unsigned long long arena_next) {
    HIP_TRY(ctr.alloc(1));
    std::unique_ptr<DevCounters> h(new DevCounters);
    memset((void *)h.get(), 0, sizeof(DevCounters));
    h->viol_key = ~0ull;
    h->arena_next = arena_next;
    HIP_TRY(hipMemcpy(ctr.p, (const void *)h.get(), sizeof(DevCounters), hipMemcpyHostToDevice));
    return MC_OK;
}
int read_counters(const DevBuf<DevCounters> &ctr, uint64_t *arena_next, uint32_t *error) {
    std::unique_ptr<DevCounters> h(new DevCounters);
    HIP_TRY(hipMemcpy((void *)h.get(), ctr.p, sizeof(DevCounters), hipMemcpyDeviceToHost));
    if (arena_next) *arena_next = h->arena_next;
    if (error) *error = h->error;
    return MC_OK;
}
int finish() {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return MC_OK;
}
// off[0] = 0, rising, off[t] = total from nranks on (Engine::shard_expand_finish)
int offsets_ok(const uint64_t *off, unsigned nranks, uint64_t total) {
    if (!nranks || nranks > 8 || off[0] != 0) return bad("owner offsets: 1 .. 8 ranks, starting at 0");
    for (unsigned t = 0; t < 8; ++t) if (off[t] > off[t + 1]) return bad("owner offsets fall");
    for (unsigned t = nranks; t <= 8; ++t) if (off[t] != total) return bad("owner offsets do not end at the total");
    return MC_OK;
}
// Engine::shard_materialise's plan
BlockPlan plan_of(const uint64_t *cnt, unsigned P) {
    BlockPlan plan;
    uint64_t blocks = 0;
    for (unsigned t = 0; t < 8; t++) {
        plan.blk_off[t] = blocks;
        plan.cnt[t] = t < P ? cnt[t] : 0;
        if (t < P) blocks += (cnt[t] + 63) / 64;
    }
    plan.blk_off[8] = blocks;
    for (unsigned t = P; t < 8; t++) plan.blk_off[t] = blocks;
    return plan;
}

// k_compact_buckets (packed == 0: out_len = the sum of the clamped cursors) or k_compact_packed (out_len = nranks * cap)
int compact(int packed, unsigned nranks, const uint64_t *cursors, const uint64_t *rt_fp, const uint32_t *rt_src, uint64_t subcap, uint64_t cap,
            uint64_t out_len, uint64_t *send_fp, uint32_t *pend_src, uint32_t *error, int *intact) {
    if (!nranks || nranks > 8 || !subcap) return bad("compact: 1 .. 8 ranks, a sub-bucket capacity");
    const unsigned nb = nranks * NSHARD;
    uint64_t sum = 0;
    for (unsigned b = 0; b < nb; ++b) sum += std::min(cursors[b], subcap);
    if (packed ? (cap < 2 || out_len != nranks * cap) : out_len != sum) return bad("compact: the output length does not fit the form");
    HIP_TRY(hipSetDevice(0));
    std::vector<PaddedCounter> cur(nb);
    memset((void *)cur.data(), 0, nb * sizeof(PaddedCounter));
    for (unsigned b = 0; b < nb; ++b) cur[b].v = cursors[b];
    DevBuf<PaddedCounter> d_cur;
    DevBuf<uint64_t> d_fp;
    DevBuf<uint32_t> d_src;
    DevBuf<DevCounters> ctr;
    Guarded<uint64_t> g_fp;
    Guarded<uint32_t> g_src;
    HIP_TRY(d_cur.alloc(nb));
    HIP_TRY(hipMemcpy(d_cur.p, cur.data(), nb * sizeof(PaddedCounter), hipMemcpyHostToDevice));
    HIP_TRY(d_fp.alloc(nb * subcap));
    HIP_TRY(hipMemcpy(d_fp.p, rt_fp, nb * subcap * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(d_src.alloc(nb * subcap));
    HIP_TRY(hipMemcpy(d_src.p, rt_src, nb * subcap * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (int rc = g_fp.make(send_fp, out_len)) return rc;
    if (int rc = g_src.make(pend_src, out_len)) return rc;
    if (int rc = fresh_counters(ctr, 0)) return rc;
    RouteArgs rt{nranks, d_cur.p, d_fp.p, d_src.p, subcap};
    if (packed) hipLaunchKernelGGL(k_compact_packed, dim3(64, nranks * NSHARD), dim3(256), 0, 0, rt, cap, g_fp.p(), g_src.p(), ctr.p);
    else hipLaunchKernelGGL(k_compact_buckets, dim3(64, nranks * NSHARD), dim3(256), 0, 0, rt, g_fp.p(), g_src.p());
    if (int rc = finish()) return rc;
    if (int rc = g_fp.fetch(send_fp)) return rc;
    if (int rc = g_src.fetch(pend_src)) return rc;
    if (int rc = read_counters(ctr, nullptr, error)) return rc;
    *intact = 1;
    if (int rc = g_fp.check(intact)) return rc;
    return g_src.check(intact);
}

}  // namespace

extern "C" {

unsigned xs_nshard() { return NSHARD; }
unsigned xs_dev_earena() { return DEV_EARENA; }
unsigned xs_dev_eroute() { return DEV_EROUTE; }
unsigned xs_guard() { return (unsigned)GUARD; }

// cursors[nranks * NSHARD] (bucket = owner * NSHARD + shard), rt_fp / rt_src[nranks * NSHARD][subcap].  send_fp / pend_src: out_len
// elements, handed in pre-filled and handed back.  *intact: the guard zones of both outputs are unchanged
int xs_compact_buckets(unsigned nranks, const uint64_t *cursors, const uint64_t *rt_fp, const uint32_t *rt_src, uint64_t subcap, uint64_t out_len,
                       uint64_t *send_fp, uint32_t *pend_src, int *intact) {
    uint32_t error = 0;
    return compact(0, nranks, cursors, rt_fp, rt_src, subcap, 0, out_len, send_fp, pend_src, &error, intact);
}
int xs_compact_packed(unsigned nranks, const uint64_t *cursors, const uint64_t *rt_fp, const uint32_t *rt_src, uint64_t subcap, uint64_t cap,
                      uint64_t *send_fp, uint32_t *pend_src, uint32_t *error, int *intact) {
    return compact(1, nranks, cursors, rt_fp, rt_src, subcap, cap, nranks * cap, send_fp, pend_src, error, intact);
}

// Engine::shard_materialise up to the plan: the scan (here: on the host), k_gather_range_ends, the starts from the ends, k_compact_new.
// answers / pend_src: total elements; off[9]; new_src: total elements, pre-filled, handed back; ends[nranks]
int xs_compact_new(unsigned nranks, const uint8_t *answers, uint64_t total, const uint64_t *off, const uint32_t *pend_src, uint32_t *new_src,
                   uint64_t *ends, int *intact) {
    if (int rc = offsets_ok(off, nranks, total)) return rc;
    if (!total || total >= (1ull << 31)) return bad("compact_new: 1 .. 2^31 - 1 candidates");
    HIP_TRY(hipSetDevice(0));
    std::vector<uint32_t> incl(total);
    uint32_t run = 0;
    for (uint64_t i = 0; i < total; ++i) incl[i] = run += answers[i] ? 1u : 0u;
    DevBuf<uint8_t> d_ans;
    DevBuf<uint32_t> d_pend;
    Guarded<uint32_t> g_incl, g_new;
    Guarded<unsigned long long> g_ends;
    std::vector<unsigned long long> h_ends(nranks, 0xa7a7a7a7a7a7a7a7ull);
    HIP_TRY(d_ans.alloc(total));
    HIP_TRY(hipMemcpy(d_ans.p, answers, total, hipMemcpyHostToDevice));
    HIP_TRY(d_pend.alloc(total));
    HIP_TRY(hipMemcpy(d_pend.p, pend_src, total * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (int rc = g_incl.make(incl.data(), total)) return rc;
    if (int rc = g_new.make(new_src, total)) return rc;
    if (int rc = g_ends.make(h_ends.data(), nranks)) return rc;
    OwnerOffsets offs, start;
    for (unsigned t = 0; t <= 8; t++) { offs.off[t] = off[t]; start.off[t] = 0; }
    hipLaunchKernelGGL(k_gather_range_ends, dim3(1), dim3(64), 0, 0, (const uint32_t *)g_incl.p(), offs, nranks, g_ends.p());
    if (int rc = finish()) return rc;
    if (int rc = g_ends.fetch(h_ends.data())) return rc;
    for (unsigned t = 0; t < nranks; t++) {
        start.off[t] = t ? h_ends[t - 1] : 0;
        ends[t] = h_ends[t];
    }
    const unsigned bx = (unsigned)((total + 255) / 256);
    hipLaunchKernelGGL(k_compact_new, dim3(bx), dim3(256), 0, 0, (const uint8_t *)d_ans.p, (const uint32_t *)g_incl.p(), (const uint32_t *)d_pend.p, total,
                       offs, start, nranks, g_new.p());
    if (int rc = finish()) return rc;
    if (int rc = g_new.fetch(new_src)) return rc;
    *intact = 1;
    if (int rc = g_incl.check(intact)) return rc;
    if (int rc = g_ends.check(intact)) return rc;
    return g_new.check(intact);
}

// k_send_parents over Engine::shard_materialise's plan for cnt[nranks]; new_src: total elements; send_parents: out_len >= the sum of the
// counts, pre-filled, handed back
int xs_send_parents(unsigned nranks, const uint32_t *new_src, uint64_t total, const uint64_t *off, const uint64_t *cnt, uint64_t chunk_base,
                    uint64_t *send_parents, uint64_t out_len, int *intact) {
    if (int rc = offsets_ok(off, nranks, total)) return rc;
    uint64_t moved = 0;
    for (unsigned t = 0; t < nranks; ++t) {
        if (cnt[t] > off[t + 1] - off[t]) return bad("send_parents: more states than the owner's range holds");
        moved += cnt[t];
    }
    if (!moved || out_len < moved) return bad("send_parents: nothing moved, or the output is shorter than what moved");
    HIP_TRY(hipSetDevice(0));
    DevBuf<uint32_t> d_new;
    Guarded<uint64_t> g_par;
    HIP_TRY(d_new.alloc(total));
    HIP_TRY(hipMemcpy(d_new.p, new_src, total * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (int rc = g_par.make(send_parents, out_len)) return rc;
    OwnerOffsets offs;
    for (unsigned t = 0; t <= 8; t++) offs.off[t] = off[t];
    hipLaunchKernelGGL(k_send_parents, dim3((unsigned)((moved + 255) / 256)), dim3(256), 0, 0, (const uint32_t *)d_new.p, chunk_base, offs,
                       plan_of(cnt, nranks), nranks, g_par.p());
    if (int rc = finish()) return rc;
    if (int rc = g_par.fetch(send_parents)) return rc;
    *intact = 1;
    return g_par.check(intact);
}

// Engine::shard_ingest: k_ingest, then k_bump_arena_next.  arena: arena_len words (whole 64-state blocks that hold arena_cap states),
// parent: arena_cap elements; both handed in and handed back.  recv_blocks: whole blocks for n states
int xs_ingest(int words, uint64_t *arena, uint64_t arena_len, uint64_t arena_cap, uint64_t arena_next, const uint64_t *recv_blocks, uint64_t n,
              uint32_t *parent, uint64_t *arena_next_out, uint32_t *error, int *intact) {
    if (words < 1 || !n || !arena_cap || arena_len != (arena_cap + 63) / 64 * 64 * (uint64_t)words) return bad("ingest: bad shape");
    if (arena_next > arena_cap) return bad("ingest: arena_next beyond the arena");
    HIP_TRY(hipSetDevice(0));
    const uint64_t recv_len = (n + 63) / 64 * 64 * (uint64_t)words;
    DevBuf<uint64_t> d_recv;
    DevBuf<DevCounters> ctr;
    Guarded<uint64_t> g_arena;
    Guarded<uint32_t> g_parent;
    HIP_TRY(d_recv.alloc(recv_len));
    HIP_TRY(hipMemcpy(d_recv.p, recv_blocks, recv_len * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (int rc = g_arena.make(arena, arena_len)) return rc;
    if (int rc = g_parent.make(parent, arena_cap)) return rc;
    if (int rc = fresh_counters(ctr, arena_next)) return rc;
    hipLaunchKernelGGL(k_ingest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, g_arena.p(), words, (const uint64_t *)d_recv.p, n, arena_cap,
                       g_parent.p(), ctr.p);
    hipLaunchKernelGGL(k_bump_arena_next, dim3(1), dim3(1), 0, 0, ctr.p, (const uint32_t *)nullptr, (unsigned long long)n, (unsigned long long)arena_cap);
    if (int rc = finish()) return rc;
    if (int rc = g_arena.fetch(arena)) return rc;
    if (int rc = g_parent.fetch(parent)) return rc;
    if (int rc = read_counters(ctr, arena_next_out, error)) return rc;
    *intact = 1;
    if (int rc = g_arena.check(intact)) return rc;
    return g_parent.check(intact);
}

// k_ingest_parents for the n states below arena_next; parent / pslot / prank: len elements, handed in and handed back
int xs_ingest_parents(const uint64_t *recv_parents, uint64_t n, unsigned src_rank, uint64_t arena_next, uint64_t len, uint32_t *parent, uint16_t *pslot,
                      uint8_t *prank, int *intact) {
    if (!n || n > arena_next || arena_next > len) return bad("ingest_parents: the n states below arena_next must lie inside the columns");
    HIP_TRY(hipSetDevice(0));
    DevBuf<uint64_t> d_recv;
    DevBuf<DevCounters> ctr;
    Guarded<uint32_t> g_parent;
    Guarded<uint16_t> g_pslot;
    Guarded<uint8_t> g_prank;
    HIP_TRY(d_recv.alloc(n));
    HIP_TRY(hipMemcpy(d_recv.p, recv_parents, n * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (int rc = g_parent.make(parent, len)) return rc;
    if (int rc = g_pslot.make(pslot, len)) return rc;
    if (int rc = g_prank.make(prank, len)) return rc;
    if (int rc = fresh_counters(ctr, arena_next)) return rc;
    hipLaunchKernelGGL(k_ingest_parents, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const uint64_t *)d_recv.p, n, src_rank, g_parent.p(),
                       g_pslot.p(), g_prank.p(), (const DevCounters *)ctr.p);
    if (int rc = finish()) return rc;
    if (int rc = g_parent.fetch(parent)) return rc;
    if (int rc = g_pslot.fetch(pslot)) return rc;
    if (int rc = g_prank.fetch(prank)) return rc;
    *intact = 1;
    if (int rc = g_parent.check(intact)) return rc;
    if (int rc = g_pslot.check(intact)) return rc;
    return g_prank.check(intact);
}

// k_bump_arena_next alone; on_device != 0: the count is read from device memory (Engine::shard_keep), else passed by value (shard_ingest)
int xs_bump_arena_next(uint64_t arena_next, uint64_t n, int on_device, uint64_t arena_cap, uint64_t *arena_next_out, uint32_t *error) {
    if (on_device && (n >> 32)) return bad("bump: a count on the device has 32 bits");
    HIP_TRY(hipSetDevice(0));
    DevBuf<DevCounters> ctr;
    DevBuf<uint32_t> d_n;
    const uint32_t n32 = (uint32_t)n;
    HIP_TRY(d_n.alloc(1));
    HIP_TRY(hipMemcpy(d_n.p, &n32, sizeof n32, hipMemcpyHostToDevice));
    if (int rc = fresh_counters(ctr, arena_next)) return rc;
    // (by value with the count on the device ignored, or the other way round: the argument the form does not use is a wrong one)
    hipLaunchKernelGGL(k_bump_arena_next, dim3(1), dim3(1), 0, 0, ctr.p, on_device ? (const uint32_t *)d_n.p : (const uint32_t *)nullptr,
                       on_device ? ~0ull : (unsigned long long)n, (unsigned long long)arena_cap);
    if (int rc = finish()) return rc;
    return read_counters(ctr, arena_next_out, error);
}

// k_gather_states: `count` states from `first` of an arena of arena_len words into out (count * words, pre-filled, handed back)
int xs_gather_states(int words, const uint64_t *arena, uint64_t arena_len, uint64_t first, uint64_t count, uint64_t *out, int *intact) {
    if (words < 1 || !count || arena_len % (64 * (uint64_t)words) || first + count > arena_len / words) return bad("gather_states: bad shape");
    HIP_TRY(hipSetDevice(0));
    DevBuf<uint64_t> d_arena;
    Guarded<uint64_t> g_out;
    HIP_TRY(d_arena.alloc(arena_len));
    HIP_TRY(hipMemcpy(d_arena.p, arena, arena_len * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (int rc = g_out.make(out, count * words)) return rc;
    hipLaunchKernelGGL(k_gather_states, dim3((unsigned)((count * words + 255) / 256)), dim3(256), 0, 0, (const uint64_t *)d_arena.p, words, first, count,
                       g_out.p());
    if (int rc = finish()) return rc;
    if (int rc = g_out.fetch(out)) return rc;
    *intact = 1;
    return g_out.check(intact);
}

}  // extern "C"
