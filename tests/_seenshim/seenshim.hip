// seenshim.hip — a test-only driver of the product's seen-set code (tla_rust_amd/csrc/engine_kernels.h: seen_insert_t in its plain, blind
// and pre-loaded forms, seen_insert_slow, k_probe, k_probe_packed, k_insert; graph.h: seen_find) on fingerprints that no model produced
// (tests/seenshim.py, tests/seenmodel.py).  A library of its own: nothing of libtlamc.so is linked and no spec template is instantiated.
// The product's headers are included unchanged, in engine.hip's order.  The kernels that take plain arrays are launched as they are; the
// device FUNCTIONS that have no such door get one thin kernel each: one lane per key, the call, the answer and the error bits stored.
// With -DSEENSHIM_HOST (g++, no HIP) only graph.h is compiled: seen_find on the host, over a table in host memory.
#if defined(SEENSHIM_HOST)
#include "graph.h"

extern "C" void ssh_find(const uint64_t *table, uint64_t nbuckets, int sparse, const uint64_t *keys, uint64_t n, uint64_t *pos) {
    const uint64_t seen = sparse ? (nbuckets | mc::GRAPH_SEEN_SPARSE) : nbuckets;
    for (uint64_t i = 0; i < n; ++i) pos[i] = mc::seen_find(table, seen, keys[i]);
}
extern "C" int ssh_sparse_slots() { return MC_SPARSE_SLOTS; }
extern "C" int ssh_probe_cap() { return mc::GRAPH_PROBE_CAP; }
#else
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
#include "graph.h"

static std::string g_error;
extern "C" void mc_set_error_internal(const char *msg) { g_error = msg ? msg : ""; }
extern "C" const char *ss_last_error() { return g_error.c_str(); }

namespace {
using namespace mc;

static_assert(GRAPH_SEEN_SPARSE == SEEN_SPARSE, "graph.h and engine_kernels.h disagree about the table's mode bit");

enum : int { F_PLAIN = 0, F_BLIND = 1, F_PRE = 2, F_SLOW = 3, F_KPROBE = 4 };

template <int SLOTS, int FORM>
__device__ __forceinline__ bool insert_one(uint64_t *table, uint64_t nbuckets, uint64_t fp, unsigned &err) {
    if constexpr (FORM == F_PLAIN) return seen_insert_t<SLOTS>(table, nbuckets, fp, err);
    else if constexpr (FORM == F_BLIND) return seen_insert_t<SLOTS, true>(table, nbuckets, fp, err);
    else if constexpr (FORM == F_PRE) {
        unsigned long long pre[SLOTS];
        seen_load_home<SLOTS>(table, nbuckets, fp, pre);
        return seen_insert_t<SLOTS, false, true>(table, nbuckets, fp, err, pre);
    } else {
        const unsigned r = seen_insert_slow(table, SLOTS == 8 ? nbuckets : (nbuckets | SEEN_SPARSE), fp);
        if (r & 2u) err |= DEV_ETABLE;
        return (r & 1u) != 0;
    }
}
// one lane per key
template <int SLOTS, int FORM>
__global__ void __launch_bounds__(256)
k_thin(const uint64_t *__restrict__ fps, uint64_t n, uint64_t *table, uint64_t nbuckets, uint8_t *__restrict__ answers, uint32_t *__restrict__ errs) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned err = 0;
    const bool nw = insert_one<SLOTS, FORM>(table, nbuckets, fps[i], err);
    answers[i] = nw ? 1 : 0;
    errs[i] = err;
}
// one at a time: a single lane inserts the keys in order
template <int SLOTS, int FORM>
__global__ void __launch_bounds__(64)
k_thin_serial(const uint64_t *__restrict__ fps, uint64_t n, uint64_t *table, uint64_t nbuckets, uint8_t *__restrict__ answers, uint32_t *__restrict__ errs) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (uint64_t i = 0; i < n; ++i) {
        unsigned err = 0;
        const bool nw = insert_one<SLOTS, FORM>(table, nbuckets, fps[i], err);
        answers[i] = nw ? 1 : 0;
        errs[i] = err;
        __threadfence();
    }
}
__global__ void __launch_bounds__(256)
k_find(const uint64_t *__restrict__ fps, uint64_t n, const uint64_t *__restrict__ table, uint64_t seen, uint64_t *__restrict__ pos) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) pos[i] = seen_find(table, seen, fps[i]);
}

template <class T>
int dev_alloc(DevBuf<T> &b, uint64_t count) {
    HIP_TRY(b.alloc(count ? count : 1));
    return MC_OK;
}
template <class T>
int upload(DevBuf<T> &b, const T *src, uint64_t count) {
    if (int rc = dev_alloc(b, count)) return rc;
    if (count) HIP_TRY(hipMemcpy(b.p, src, count * sizeof(T), hipMemcpyHostToDevice));
    return MC_OK;
}
template <class T>
int download(T *dst, const DevBuf<T> &b, uint64_t count) {
    if (count) HIP_TRY(hipMemcpy(dst, b.p, count * sizeof(T), hipMemcpyDeviceToHost));
    return MC_OK;
}
int bad(const char *what) { set_error(std::string("seenshim: ") + what); return MC_EBADCFG; }
// the forms the product has: 8 slots, or MC_SPARSE_SLOTS with the mode bit
int slots_ok(int slots) { return slots == 8 || slots == MC_SPARSE_SLOTS ? MC_OK : bad("slots must be 8 or MC_SPARSE_SLOTS"); }
uint64_t seen_arg(int slots, uint64_t nbuckets) { return slots == 8 ? nbuckets : (nbuckets | SEEN_SPARSE); }
unsigned blocks_of(uint64_t n) { return (unsigned)((n + 255) / 256); }

// a zeroed counter block with max_slots set
int fresh_counters(DevBuf<DevCounters> &ctr, unsigned max_slots) {
    if (int rc = dev_alloc(ctr, 1)) return rc;
    DevCounters *h = new DevCounters;
    memset((void *)h, 0, sizeof *h);
    h->max_slots = max_slots;
    h->viol_key = ~0ull;
    const hipError_t e = hipMemcpy(ctr.p, h, sizeof *h, hipMemcpyHostToDevice);
    delete h;
    HIP_TRY(e);
    return MC_OK;
}

template <int SLOTS>
int launch_thin(int form, int serial, const uint64_t *fps, uint64_t n, uint64_t *table, uint64_t nbuckets, uint8_t *answers, uint32_t *errs) {
#define SS_FORM(F)                                                                                                              \
    case F:                                                                                                                     \
        if (serial) hipLaunchKernelGGL((k_thin_serial<SLOTS, F>), dim3(1), dim3(64), 0, 0, fps, n, table, nbuckets, answers, errs); \
        else hipLaunchKernelGGL((k_thin<SLOTS, F>), dim3(blocks_of(n)), dim3(256), 0, 0, fps, n, table, nbuckets, answers, errs); \
        break;
    switch (form) {
        SS_FORM(F_PLAIN)
        SS_FORM(F_BLIND)
        SS_FORM(F_PRE)
        SS_FORM(F_SLOW)
        default: return bad("no such form");
    }
#undef SS_FORM
    HIP_TRY(hipGetLastError());
    return MC_OK;
}

}  // namespace

extern "C" {

int ss_sparse_slots() { return MC_SPARSE_SLOTS; }
unsigned ss_dev_etable() { return DEV_ETABLE; }

// Inserts keys[0..n) into `table` (nbuckets * slots words of host memory: uploaded, probed, downloaded).  form: 0 seen_insert_t,
// 1 its BLIND form, 2 its PRE form fed by seen_load_home, 3 seen_insert_slow, 4 the kernel k_probe.  serial != 0: one at a time, in
// order (a one-lane loop; k_probe: one launch per key).  answers[i]: 1 = new.  errs[i]: the DEV_E* bits the call raised for key i
// (k_probe: all 0); *ctr_error: the counter block's error word (k_probe alone writes it).
int ss_insert_keys(int form, int slots, int serial, uint64_t nbuckets, uint64_t *table, const uint64_t *keys, uint64_t n, uint8_t *answers, uint32_t *errs,
                   uint32_t *ctr_error) {
    if (int rc = slots_ok(slots)) return rc;
    if (!nbuckets || (nbuckets >> 32)) return bad("the bucket count must be in 1 .. 2^32 - 1");
    HIP_TRY(hipSetDevice(0));
    DevBuf<uint64_t> d_table, d_keys;
    DevBuf<uint8_t> d_ans;
    DevBuf<uint32_t> d_errs;
    DevBuf<DevCounters> ctr;
    if (int rc = upload(d_table, table, nbuckets * slots)) return rc;
    if (int rc = upload(d_keys, keys, n)) return rc;
    if (int rc = dev_alloc(d_ans, n)) return rc;
    if (int rc = dev_alloc(d_errs, n)) return rc;
    HIP_TRY(hipMemset(d_ans.p, 0xee, n ? n : 1));
    HIP_TRY(hipMemset(d_errs.p, 0, (n ? n : 1) * sizeof(uint32_t)));
    if (int rc = fresh_counters(ctr, 0)) return rc;
    if (n) {
        if (form == F_KPROBE) {
            const uint64_t seen = seen_arg(slots, nbuckets);
            if (serial) {
                for (uint64_t i = 0; i < n; ++i) hipLaunchKernelGGL(k_probe, dim3(1), dim3(256), 0, 0, d_keys.p + i, (uint64_t)1, d_table.p, seen, d_ans.p + i, ctr.p);
            } else {
                hipLaunchKernelGGL(k_probe, dim3(blocks_of(n)), dim3(256), 0, 0, d_keys.p, n, d_table.p, seen, d_ans.p, ctr.p);
            }
            HIP_TRY(hipGetLastError());
        } else if (slots == 8) {
            if (int rc = launch_thin<8>(form, serial, d_keys.p, n, d_table.p, nbuckets, d_ans.p, d_errs.p)) return rc;
        } else {
            if (int rc = launch_thin<MC_SPARSE_SLOTS>(form, serial, d_keys.p, n, d_table.p, nbuckets, d_ans.p, d_errs.p)) return rc;
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = download(table, d_table, nbuckets * slots)) return rc;
    if (int rc = download(answers, d_ans, n)) return rc;
    if (int rc = download(errs, d_errs, n)) return rc;
    HIP_TRY(hipMemcpy(ctr_error, &ctr.p->error, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MC_OK;
}

// k_probe_packed over nranks buckets of `cap` words each (word 0 of a bucket: its count); answers: nranks * cap bytes, pre-filled with 0xee
int ss_probe_packed(int slots, uint64_t nbuckets, uint64_t *table, const uint64_t *fps, uint64_t cap, unsigned nranks, uint8_t *answers, uint32_t *ctr_error) {
    if (int rc = slots_ok(slots)) return rc;
    if (!nbuckets || (nbuckets >> 32) || !cap || !nranks) return bad("ss_probe_packed: empty");
    HIP_TRY(hipSetDevice(0));
    DevBuf<uint64_t> d_table, d_fps;
    DevBuf<uint8_t> d_ans;
    DevBuf<DevCounters> ctr;
    const uint64_t total = cap * nranks;
    if (int rc = upload(d_table, table, nbuckets * slots)) return rc;
    if (int rc = upload(d_fps, fps, total)) return rc;
    if (int rc = dev_alloc(d_ans, total)) return rc;
    HIP_TRY(hipMemset(d_ans.p, 0xee, total));
    if (int rc = fresh_counters(ctr, 0)) return rc;
    // (engine.hip's grid: the workgroups of one bucket times the ranks)
    hipLaunchKernelGGL(k_probe_packed, dim3(blocks_of(cap) * nranks), dim3(256), 0, 0, d_fps.p, cap, nranks, d_table.p, seen_arg(slots, nbuckets), d_ans.p, ctr.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = download(table, d_table, nbuckets * slots)) return rc;
    if (int rc = download(answers, d_ans, total)) return rc;
    HIP_TRY(hipMemcpy(ctr_error, &ctr.p->error, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MC_OK;
}

// k_insert over a slot-major candidate matrix (grid_y rows of row_stride words; ncols columns are looked at, nsl[col] slots of each, rows
// below max_slots).  newlist: newlist_len words, handed in pre-filled and handed back.  out[0] n_new[0], out[1] cells[0], out[2] error
int ss_k_insert(int slots, uint64_t nbuckets, uint64_t *table, const uint64_t *cand, uint64_t row_stride, uint64_t ncols, unsigned grid_y, unsigned max_slots,
                const uint16_t *nsl, uint32_t *newlist, uint64_t newlist_len, uint64_t *out) {
    if (int rc = slots_ok(slots)) return rc;
    if (!nbuckets || (nbuckets >> 32) || !ncols || ncols > row_stride || !grid_y || grid_y > 256 || ncols >= (1u << 24)) return bad("ss_k_insert: bad shape");
    uint64_t cands = 0;   // the new-list must hold every candidate the kernel may find new
    for (uint64_t c = 0; c < ncols; ++c) cands += std::min<uint64_t>(nsl[c], std::min(grid_y, max_slots));
    if (newlist_len < cands) return bad("ss_k_insert: the new-list is shorter than the candidates");
    HIP_TRY(hipSetDevice(0));
    DevBuf<uint64_t> d_table, d_cand;
    DevBuf<uint16_t> d_nsl;
    DevBuf<uint32_t> d_new;
    DevBuf<DevCounters> ctr;
    if (int rc = upload(d_table, table, nbuckets * slots)) return rc;
    if (int rc = upload(d_cand, cand, row_stride * grid_y)) return rc;
    if (int rc = upload(d_nsl, nsl, ncols)) return rc;
    if (int rc = upload(d_new, newlist, newlist_len)) return rc;
    if (int rc = fresh_counters(ctr, max_slots)) return rc;
    hipLaunchKernelGGL(k_insert, dim3(blocks_of(ncols), grid_y), dim3(256), 0, 0, d_cand.p, row_stride, ncols, d_nsl.p, d_table.p, seen_arg(slots, nbuckets), d_new.p, ctr.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = download(table, d_table, nbuckets * slots)) return rc;
    if (int rc = download(newlist, d_new, newlist_len)) return rc;
    std::unique_ptr<DevCounters> h(new DevCounters);
    HIP_TRY(hipMemcpy((void *)h.get(), ctr.p, sizeof(DevCounters), hipMemcpyDeviceToHost));
    out[0] = h->n_new[0].v;
    out[1] = h->cells[0].v;
    out[2] = h->error;
    return MC_OK;
}

// graph.h's seen_find on the device, one lane per key
int ss_find(int slots, uint64_t nbuckets, const uint64_t *table, const uint64_t *keys, uint64_t n, uint64_t *pos) {
    if (int rc = slots_ok(slots)) return rc;
    if (!nbuckets || (nbuckets >> 32)) return bad("the bucket count must be in 1 .. 2^32 - 1");
    HIP_TRY(hipSetDevice(0));
    DevBuf<uint64_t> d_table, d_keys, d_pos;
    if (int rc = upload(d_table, table, nbuckets * slots)) return rc;
    if (int rc = upload(d_keys, keys, n)) return rc;
    if (int rc = dev_alloc(d_pos, n)) return rc;
    if (n) {
        hipLaunchKernelGGL(k_find, dim3(blocks_of(n)), dim3(256), 0, 0, d_keys.p, n, d_table.p, seen_arg(slots, nbuckets), d_pos.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipDeviceSynchronize());
    return download(pos, d_pos, n);
}

}  // extern "C"
#endif
