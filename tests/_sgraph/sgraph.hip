// sgraph.hip — a test-only driver of mc::StateGraph (tla_rust_amd/csrc/state_graph.h): it hands the product's state_graph.hip, compiled
// beside it into a library of its own, CSR arrays that no search of a model produced (tests/sgraph.py, tests/randgraph.py).  No kernel
// lives here and nothing of libtlamc.so is linked: what runs on the device is engine_live.h alone.  The order of the calls is the
// engine's (engine.hip: liveness_run, predicates_build): the components first — StateGraph::scc() releases lv.proc and lv.pred —,
// then the edges' processes and the predicate bits, uploaded here where the engine enqueues k_live_proc / k_live_pred, once per
// component build; then StateGraph::live_check, whose refusals of a bad query (live_query.h) are the product's own.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "state_graph.h"

static std::string g_error;
extern "C" void mc_set_error_internal(const char *msg) { g_error = msg ? msg : ""; }
extern "C" const char *sg_last_error() { return g_error.c_str(); }

namespace {

struct Sg {
    mc::StateGraph g;
    mc::Stream stream;
    bool has_proc = false, has_pred = false;
    std::vector<int8_t> proc;      // host copies: uploaded after every component build
    std::vector<uint32_t> pred;
};

template <class T>
int upload(mc::DevBuf<T> &buf, const T *src, uint64_t count, const char *what) {
    if (int rc = mc::graph_alloc(buf, count, what, "sgraph")) return rc;
    if (count) HIP_TRY(hipMemcpy(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice));
    return MC_OK;
}

int create(Sg &s, uint64_t n, uint64_t edges, uint64_t init_states, const uint64_t *offsets, const uint32_t *dst, const int8_t *proc, const uint32_t *pred) {
    if (n + 1 > 0x7fffffffull) { mc::set_error("sgraph: at most 2^31 - 2 states"); return MC_EBADCFG; }
    if (offsets[0] != 0 || offsets[n] != edges) { mc::set_error("sgraph: offsets[0] is not 0 or offsets[n] is not the number of edges"); return MC_EBADCFG; }
    for (uint64_t v = 0; v < n; ++v)
        if (offsets[v] > offsets[v + 1]) { mc::set_error("sgraph: offsets fall at state " + std::to_string(v)); return MC_EBADCFG; }
    // (the kernels skip a successor beyond the states; the fairness pass and the trace do not expect one: a built graph never holds it)
    for (uint64_t k = 0; k < edges; ++k) {
        if (dst[k] >= n) { mc::set_error("sgraph: edge " + std::to_string(k) + " ends beyond the states"); return MC_EBADCFG; }
        if (proc && (proc[k] < -1 || proc[k] >= 64)) { mc::set_error("sgraph: edge " + std::to_string(k) + " has no process in -1 .. 63"); return MC_EBADCFG; }
    }
    if (init_states > n) { mc::set_error("sgraph: more initial states than states"); return MC_EBADCFG; }
    HIP_TRY(hipSetDevice(0));
    HIP_TRY(s.stream.create());
    s.g.device = 0;
    if (int rc = upload(s.g.offsets, offsets, n + 1, "the row offsets")) return rc;
    if (int rc = upload(s.g.dst, dst, edges, "the edges' successors")) return rc;
    if (int rc = mc::graph_alloc(s.g.act, edges, "the edges' actions", "sgraph")) return rc;
    HIP_TRY(hipMemset(s.g.act.p, 0, (edges ? edges : 1) * sizeof(int16_t)));
    if (proc) { s.has_proc = true; s.proc.assign(proc, proc + edges); }
    if (pred) { s.has_pred = true; s.pred.assign(pred, pred + n); }
    memset(&s.g.info, 0, sizeof s.g.info);
    s.g.info.states = n;
    s.g.info.expanded = n;
    s.g.info.edges = edges;
    s.g.info.init_states = init_states;
    s.g.built = true;
    return MC_OK;
}

int pred_bits(Sg &s) {
    auto &lv = s.g.lv;
    if (lv.pred_built) return MC_OK;
    HIP_TRY(hipSetDevice(s.g.device));
    if (int rc = upload(lv.pred, s.pred.data(), s.g.info.states, "the predicate bits")) return rc;
    lv.pred_built = true;
    lv.npred = mc::LIVE_MAX_PREDS;   // (every bit of a word may be a predicate's)
    return MC_OK;
}
// engine.hip's liveness_run up to the call into StateGraph: the components, then what the query reads and the graph does not hold yet
int prepare(Sg &s, bool want_pred, const char *call) {
    if (!s.has_proc) { mc::set_error(std::string(call) + ": the graph was created without the edges' processes"); return MC_EBADCFG; }
    if (want_pred && !s.has_pred) { mc::set_error(std::string(call) + ": the graph was created without predicate bits"); return MC_EBADCFG; }
    auto &lv = s.g.lv;
    if (!lv.scc_built) { mc_scc_info si; if (int rc = s.g.scc(s.stream, &si)) return rc; }
    HIP_TRY(hipSetDevice(s.g.device));
    if (!lv.proc_built) {
        if (int rc = upload(lv.proc, s.proc.data(), s.g.info.edges, "the edges' processes")) return rc;
        lv.proc_built = true;
    }
    return want_pred ? pred_bits(s) : MC_OK;
}
// one check: the outputs that apply zeroed, the preparation — `more`: what a driver built on this one adds to it —, then the product's
// one entry (which refuses a bad query)
int check(Sg &s, const mc::LiveQuery &q, mc_live_info *lout, mc_live_check_info *cout, mc_live_strong_info *sout,
          int (*more)(Sg &, const mc::LiveQuery &) = nullptr) {
    const auto t0 = std::chrono::steady_clock::now();
    if (lout) memset(lout, 0, sizeof *lout);
    if (cout) memset(cout, 0, sizeof *cout);
    if (sout) memset(sout, 0, sizeof *sout);
    if (int rc = prepare(s, cout != nullptr, q.call)) return rc;
    if (more) if (int rc = more(s, q)) return rc;
    return s.g.live_check(q, s.stream, t0, lout, cout, sout);
}

}  // namespace

extern "C" {

void *sg_create(uint64_t n, uint64_t edges, uint64_t init_states, const uint64_t *offsets, const uint32_t *dst, const int8_t *proc, const uint32_t *pred) {
    if (!offsets || (edges && !dst)) { mc::set_error("sgraph: no arrays"); return nullptr; }
    Sg *s = new Sg;
    if (create(*s, n, edges, init_states, offsets, dst, proc, pred)) { delete s; return nullptr; }
    return s;
}
void sg_destroy(void *h) { delete (Sg *)h; }

int sg_scc(void *h, mc_scc_info *out) { Sg &s = *(Sg *)h; return s.g.scc(s.stream, out); }
int sg_scc_read(void *h, uint64_t first, uint64_t count, uint32_t *out) { return ((Sg *)h)->g.scc_read(first, count, out); }
int sg_live_scc_read(void *h, uint64_t first, uint64_t count, uint32_t *out) { return ((Sg *)h)->g.live_scc_read(first, count, out); }

int sg_live_check(void *h, uint64_t all, uint64_t fair, mc_live_info *out) {
    return check(*(Sg *)h, mc::LiveQuery{"sg_live_check", all, fair, 0, nullptr, -1, -1, -1, false}, out, nullptr, nullptr);
}
int sg_live_check_masked(void *h, uint64_t all, uint64_t fair, int kind, int p, int q, mc_live_check_info *out) {
    return check(*(Sg *)h, mc::LiveQuery{"sg_live_check_masked", all, fair, 0, nullptr, kind, p, q, false}, nullptr, out, nullptr);
}
// (as mc_engine_predicates: the bits are there once a check, or this call, has put them there)
int sg_pred_read(void *h, uint64_t first, uint64_t count, uint32_t *out) {
    Sg &s = *(Sg *)h;
    if (s.has_pred) if (int rc = pred_bits(s)) return rc;
    return s.g.pred_read(first, count, out);
}
int sg_live_trace(void *h, const uint64_t *level_start, size_t nlevels, uint32_t *prefix_out, size_t *nprefix_inout, uint32_t *cycle_out, size_t *ncycle_inout) {
    const std::vector<uint64_t> levels(level_start, level_start + nlevels);
    return ((Sg *)h)->g.live_trace(levels, prefix_out, nprefix_inout, cycle_out, ncycle_inout);
}

// the two scans over host arrays
int sg_scan_exclusive_u32_to_u64(const uint32_t *in, uint64_t *out, uint64_t n) {
    HIP_TRY(hipSetDevice(0));
    mc::Stream stream;
    HIP_TRY(stream.create());
    mc::DevBuf<uint32_t> d_in;
    mc::DevBuf<uint64_t> d_out;
    mc::DevBuf<char> tmp;
    if (int rc = upload(d_in, in, n, "the scan's input")) return rc;
    if (int rc = mc::graph_alloc(d_out, n, "the scan's output", "sgraph")) return rc;
    if (int rc = mc::scan_exclusive_u32_to_u64(d_in.p, d_out.p, n, tmp, stream, "sgraph")) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    if (n) HIP_TRY(hipMemcpy(out, d_out.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return MC_OK;
}
int sg_scan_answers_inclusive(const uint8_t *answers, uint32_t *incl, uint64_t n) {
    HIP_TRY(hipSetDevice(0));
    mc::Stream stream;
    HIP_TRY(stream.create());
    mc::DevBuf<uint8_t> d_in;
    mc::DevBuf<uint32_t> d_out;
    mc::DevBuf<char> tmp;
    if (int rc = upload(d_in, answers, n, "the scan's input")) return rc;
    if (int rc = mc::graph_alloc(d_out, n, "the scan's output", "sgraph")) return rc;
    if (int rc = mc::scan_answers_inclusive(d_in.p, d_out.p, n, tmp, stream)) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    if (n) HIP_TRY(hipMemcpy(incl, d_out.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MC_OK;
}

}  // extern "C"
