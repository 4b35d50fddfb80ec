// state_graph.hip — the HOST half of everything that consumes the state graph's CSR arrays (state_graph.h): the reads, the strongly
// connected components, the liveness checks and their counterexample.  One object in the library: no lowering is named below this line,
// and the engines of all of them — the units of engine.hip, the unit of generated code built at load time — call in here.  The
// kernels and the two device scans are engine_live.h's.  The checks have ONE entry, live_check: it refuses or normalises the query
// (live_query.h), starts lv.last — what live_trace and live_scc_read know of the last check — afresh, and runs the single pass
// (live_single) or the refinement (live_refined) over shared pieces: live_arrays, live_clear, live_reduce, live_termination, live_reach_tail.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "state_graph.h"
#include "engine_live.h"   // k_scc_* / k_live_*: the kernels; liveness.h: the rule the counterexample builder runs too

namespace mc {

// ------------------------------------------------------------------------------- the graph's rows
int StateGraph::read(uint64_t first, uint64_t count, uint64_t *offsets_out, uint32_t *dst_out, int32_t *action_out, size_t *nedges_inout) {
    if (!built) { set_error("mc_engine_graph_read: no graph (mc_engine_graph builds it; the next search releases it)"); return MC_ESTATE; }
    if (first > info.states || count > info.states - first) { set_error("mc_engine_graph_read: range beyond the graph's states"); return MC_EBADCFG; }
    HIP_TRY(hipSetDevice(device));
    std::vector<uint64_t> off((size_t)count + 1);
    HIP_TRY(hipMemcpy(off.data(), offsets.p + first, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    const uint64_t e0 = off[0], ne = off[count] - e0;
    if (ne > *nedges_inout || !offsets_out || (ne && (!dst_out || !action_out))) {
        *nedges_inout = (size_t)ne;
        set_error("mc_engine_graph_read: buffer too small (" + std::to_string((unsigned long long)ne) + " edges)");
        return MC_EBADCFG;
    }
    for (uint64_t k = 0; k <= count; k++) offsets_out[k] = off[k] - e0;
    if (ne) {
        std::vector<int16_t> a16((size_t)ne);
        HIP_TRY(hipMemcpy(dst_out, dst.p + e0, ne * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(a16.data(), act.p + e0, ne * sizeof(int16_t), hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < ne; k++) action_out[k] = a16[k];
    }
    *nedges_inout = (size_t)ne;
    return MC_OK;
}

// ------------------------------------------------------------------------------- components and fairness (engine_live.h)
// One kernel over all states: the launches of this section differ in the kernel and its arguments only.
template <class K, class... A>
static void live_launch(hipStream_t stream, K kernel, uint64_t n, A... args) {
    if (n) hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, args...);
}
// SCC_BATCH sweeps, then one read of the flag; until a whole batch changed nothing.  `rounds` counts the sweeps launched.
// max_rounds: a fixed point that needs more sweeps than that "did not converge" (MC_ESTATE); 0 = no bound
template <class F>
static int live_fixed_point(hipStream_t stream, unsigned *flag, uint32_t &rounds, F &&sweep, uint64_t max_rounds = 0, const char *what = "") {
    for (;;) {
        if (max_rounds && rounds > max_rounds) { set_error(std::string(what) + " did not converge after " + std::to_string(rounds) + " sweeps"); return MC_ESTATE; }
        HIP_TRY(hipMemsetAsync(flag, 0, sizeof(unsigned), stream));
        for (int k = 0; k < SCC_BATCH; ++k) sweep();
        rounds += SCC_BATCH;
        unsigned h = 0;
        HIP_TRY(hipMemcpyAsync(&h, flag, sizeof h, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (!h) return MC_OK;
    }
}
int StateGraph::scc(hipStream_t stream, mc_scc_info *out) {
    lv.release();
    const uint64_t n = info.states;
    HIP_TRY(hipSetDevice(device));
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = scc_build(n, stream);
    if (rc) { lv.release(); return rc; }
    lv.sinfo.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    lv.scc_built = true;
    *out = lv.sinfo;
    return MC_OK;
}
int StateGraph::scc_build(uint64_t n, hipStream_t stream) {
    DevBuf<uint32_t> indeg;   // build-time only: the in-degrees, then the fill's cursors
    DevBuf<char> scan_tmp;
    int rc;
    if ((rc = graph_alloc(indeg, n + 1, "the in-degrees", "mc_engine_scc"))) return rc;
    if ((rc = graph_alloc(lv.toff, n + 1, "the transpose's row offsets", "mc_engine_scc"))) return rc;
    const uint64_t *off = offsets.p;
    const uint32_t *dst = this->dst.p;
    // ---- transpose
    HIP_TRY(hipMemsetAsync(indeg, 0, (n + 1) * sizeof(uint32_t), stream));
    live_launch(stream, k_live_indegree, n, off, dst, indeg.p);
    HIP_TRY(hipGetLastError());
    if ((rc = scan_exclusive_u32_to_u64(indeg.p, lv.toff.p, n + 1, scan_tmp, stream, "mc_engine_scc"))) return rc;
    uint64_t tedges = 0;
    HIP_TRY(hipMemcpyAsync(&tedges, lv.toff.p + n, sizeof tedges, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if ((rc = graph_alloc(lv.tsrc, tedges, "the transpose's sources", "mc_engine_scc"))) return rc;
    HIP_TRY(hipMemsetAsync(indeg, 0, (n + 1) * sizeof(uint32_t), stream));
    live_launch(stream, k_live_tfill, n, off, dst, (const uint64_t *)lv.toff.p, indeg.p, lv.tsrc.p);
    HIP_TRY(hipGetLastError());
    return scc_components(n, stream, -1, lv.scc, lv.size, lv.sinfo);
}
int StateGraph::scc_components(uint64_t n, hipStream_t stream, int mask_q, DevBuf<uint32_t> &scc_buf, DevBuf<uint32_t> &size_buf, mc_scc_info &info,
                               const uint8_t *open) {
    DevBuf<unsigned> flag;
    DevBuf<LiveCounters> d_lc;
    int rc;
    if ((rc = graph_alloc(scc_buf, n, "the component ids", "mc_engine_scc"))) return rc;
    if ((rc = graph_alloc(size_buf, n, "the colours", "mc_engine_scc"))) return rc;
    if ((rc = graph_alloc(flag, 1, "the fixed-point flag", "mc_engine_scc"))) return rc;
    if ((rc = graph_alloc(d_lc, 1, "the counters", "mc_engine_scc"))) return rc;
    const uint64_t *off = offsets.p;
    const uint32_t *dst = this->dst.p;
    // ---- trim and colouring until no state is live
    const uint64_t *toff = lv.toff.p;
    const uint32_t *tsrc = lv.tsrc.p;
    uint32_t *scc = scc_buf.p, *colour = size_buf.p;
    HIP_TRY(hipMemsetAsync(scc, 0xff, n * sizeof(uint32_t), stream));
    if (mask_q >= 0) live_launch(stream, k_scc_mask, n, (const uint32_t *)lv.pred.p, LiveCheck{LIVE_INF_OFTEN, -1, mask_q}, scc);
    if (open) live_launch(stream, k_scc_open, n, open, scc);
    uint32_t trim_rounds = 0, colour_rounds = 0, back_rounds = 0, passes = 0;
    for (; n;) {
        if ((rc = live_fixed_point(stream, flag.p, trim_rounds, [&] { live_launch(stream, k_scc_trim, n, off, dst, toff, tsrc, scc, flag.p); }))) return rc;
        unsigned live = 0;
        HIP_TRY(hipMemsetAsync(flag, 0, sizeof(unsigned), stream));
        live_launch(stream, k_scc_colour_init, n, (const uint32_t *)scc, colour, flag.p);
        HIP_TRY(hipMemcpyAsync(&live, flag, sizeof live, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (!live) break;
        ++passes;
        if ((rc = live_fixed_point(stream, flag.p, colour_rounds, [&] { live_launch(stream, k_scc_colour, n, toff, tsrc, (const uint32_t *)scc, colour, flag.p); }))) return rc;
        live_launch(stream, k_scc_roots, n, scc, (const uint32_t *)colour);
        if ((rc = live_fixed_point(stream, flag.p, back_rounds, [&] { live_launch(stream, k_scc_back, n, off, dst, scc, (const uint32_t *)colour, flag.p); }))) return rc;
    }
    // ---- ids: the least index of the component; sizes; statistics (the colour array serves as `least`, then as `size`)
    LiveCounters lc;
    memset(&lc, 0, sizeof lc);
    lc.first_root = ~0u;
    HIP_TRY(hipMemcpyAsync(d_lc, &lc, sizeof lc, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(colour, 0xff, (n ? n : 1) * sizeof(uint32_t), stream));
    live_launch(stream, k_scc_least, n, (const uint32_t *)scc, colour);
    live_launch(stream, k_scc_renumber, n, scc, (const uint32_t *)colour);
    HIP_TRY(hipMemsetAsync(colour, 0, (n ? n : 1) * sizeof(uint32_t), stream));
    live_launch(stream, k_scc_sizes, n, (const uint32_t *)scc, colour);
    live_launch(stream, k_scc_stats, n, (const uint32_t *)scc, (const uint32_t *)colour, d_lc.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&lc, d_lc, sizeof lc, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    memset(&info, 0, sizeof info);
    info.states = n;
    info.components = lc.components;
    info.nontrivial = lc.nontrivial;
    info.largest = lc.largest;
    info.trim_rounds = trim_rounds;
    info.colour_rounds = colour_rounds;
    info.backward_rounds = back_rounds;
    info.passes = passes;
    return MC_OK;
}
int StateGraph::scc_read(uint64_t first, uint64_t count, uint32_t *scc_out) {
    if (!built || !lv.scc_built) { set_error("mc_engine_scc_read: no components (mc_engine_scc finds them; the next search releases them)"); return MC_ESTATE; }
    if (first > info.states || count > info.states - first) { set_error("mc_engine_scc_read: range beyond the graph's states"); return MC_EBADCFG; }
    HIP_TRY(hipSetDevice(device));
    if (count) HIP_TRY(hipMemcpy(scc_out, lv.scc.p + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MC_OK;
}
int StateGraph::live_scc_read(uint64_t first, uint64_t count, uint32_t *scc_out) {
    if (!built || !lv.last.checked || (lv.last.kind < 0 && !lv.last.refined)) { set_error("mc_engine_liveness_components: no property check (mc_engine_liveness_check runs one; the next search releases it)"); return MC_ESTATE; }
    if (first > info.states || count > info.states - first) { set_error("mc_engine_liveness_components: range beyond the graph's states"); return MC_EBADCFG; }
    HIP_TRY(hipSetDevice(device));
    if (count) HIP_TRY(hipMemcpy(scc_out, (lv.last.refined ? lv.fscc.p : lv.last.mask ? lv.last.mask->scc.p : lv.scc.p) + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MC_OK;
}
int StateGraph::live_unit_read(uint64_t first, uint64_t count, int8_t *unit_out) {
    if (!built || !lv.unit_built) { set_error("mc_engine_liveness_edge_units: no units (mc_engine_liveness_units / mc_engine_liveness_check_units fill them; the next search releases them)"); return MC_ESTATE; }
    if (first > info.edges || count > info.edges - first) { set_error("mc_engine_liveness_edge_units: range beyond the graph's edges"); return MC_EBADCFG; }
    HIP_TRY(hipSetDevice(device));
    if (count) HIP_TRY(hipMemcpy(unit_out, lv.unit.p + first, count * sizeof(int8_t), hipMemcpyDeviceToHost));
    return MC_OK;
}
int StateGraph::pred_read(uint64_t first, uint64_t count, uint32_t *bits_out) {
    if (!built || !lv.pred_built) { set_error("mc_engine_predicates: no predicate bits"); return MC_ESTATE; }
    if (first > info.states || count > info.states - first) { set_error("mc_engine_predicates: range beyond the graph's states"); return MC_EBADCFG; }
    HIP_TRY(hipSetDevice(device));
    if (count) HIP_TRY(hipMemcpy(bits_out, lv.pred.p + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MC_OK;
}
// the components of G[M] for a property check: null (the full graph's) for <>[]P, else the build kept for the predicate that masks — made
// and kept here when there is none
int StateGraph::live_mask_components(int kind, int q, hipStream_t stream, const Live::Masked **mask_out, uint32_t *builds) {
    const uint64_t n = info.states;
    const Live::Masked *mask = nullptr;
    if (kind != LIVE_STABLE) {
        for (const auto &m : lv.masks) if (m->q == q) mask = m.get();
        if (!mask) {
            auto m = std::make_unique<Live::Masked>();
            m->q = q;
            mc_scc_info si;
            if (int rc = scc_components(n, stream, q, m->scc, m->size, si)) return rc;
            ++*builds;
            mask = m.get();
            lv.masks.push_back(std::move(m));
        }
    }
    *mask_out = mask;
    return MC_OK;
}
// ------------------------------------------------------------------------------- the liveness checks: ONE entry (live_query.h says which)
// After the engine's k_live_proc<S> / k_live_unit<S> / k_live_pred<S> (enqueued on `stream`): the query refused or normalised, the
// record of the last check started afresh, then the single pass of the weak entries or the refinement of the strong and unit ones.
int StateGraph::live_check(const LiveQuery &query, hipStream_t stream, std::chrono::steady_clock::time_point started, mc_live_info *lout,
                           mc_live_check_info *cout, mc_live_strong_info *sout) {
    if (int rc = live_query_check(query, lv.npred)) return rc;
    const LiveQuery q = live_query_normalised(query);
    lv.last = Live::Last{};
    lv.last.kind = q.kind;
    lv.last.p = q.p;
    lv.last.q = q.q;
    lv.last.refined = q.refine;
    lv.last.units = q.fu != nullptr;
    lv.last.fair = q.weak;
    lv.last.strong = q.strong;
    return q.refine ? live_refined(q, stream, started, lout, cout, sout) : live_single(q, stream, started, lout, cout);
}
// The arrays a query's passes write, allocated before anything of the check is enqueued (an allocation may wait for the device):
// taken / disabled / done at a component's id; a refinement's enabled, open states and refined ids; a property's distances.
int StateGraph::live_arrays(const LiveQuery &q) {
    const uint64_t n = info.states;
    int rc;
    if ((rc = graph_alloc(lv.taken, n, "the components' taken masks", q.call))) return rc;
    if ((rc = graph_alloc(lv.disabled, n, "the components' disabled masks", q.call))) return rc;
    if ((rc = graph_alloc(lv.done, n, q.term() && !q.refine ? "the components' Done flags" : "the components' target flags", q.call))) return rc;
    if (q.refine) {
        if ((rc = graph_alloc(lv.enabled, n, "the components' enabled masks", q.call))) return rc;
        if ((rc = graph_alloc(lv.open, n, "the open states", q.call))) return rc;
        if ((rc = graph_alloc(lv.fscc, n, "the refined component ids", q.call))) return rc;
        if ((rc = graph_alloc(lv.fsize, n, "the refined components' sizes", q.call))) return rc;
    }
    if (!q.term() && (rc = graph_alloc(lv.dist, n, "the distances", q.call))) return rc;
    return MC_OK;
}
// ... and the per-component ones cleared, before every reduce pass
int StateGraph::live_clear(const LiveQuery &q, hipStream_t stream) {
    const uint64_t cells = info.states ? info.states : 1;
    HIP_TRY(hipMemsetAsync(lv.taken, 0, cells * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(lv.disabled, 0, cells * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(lv.done, 0, cells * sizeof(unsigned), stream));
    if (q.refine) HIP_TRY(hipMemsetAsync(lv.enabled, 0, cells * sizeof(unsigned long long), stream));
    return MC_OK;
}
// The reduce pass over the components scc / size: the one place that picks among k_live_reduce{,_units}<MASKED> — MASKED for a property,
// _units (lv.unit in lv.proc's place, the staged table behind the arguments) for a check label by label.
void StateGraph::live_reduce(const LiveQuery &q, hipStream_t stream, const uint32_t *scc, const uint32_t *size, const LiveCheck &ck) {
    const uint32_t *pred = q.term() ? nullptr : lv.pred.p;
    const int8_t *edge_class = q.fu ? lv.unit.p : lv.proc.p;   // (the units have an array of their own: proc[] stays what a process-level check reads)
    auto go = [&](auto kernel, auto... tab) {
        live_launch(stream, kernel, (uint64_t)info.states, (const uint64_t *)offsets.p, (const uint32_t *)dst.p, edge_class, scc, size, q.all, lv.taken.p,
                    lv.disabled.p, lv.done.p, pred, ck, tab...);
    };
    const uint64_t *tab = lv.of_unit.p;
    if (q.fu) q.term() ? go(k_live_reduce_units<false>, tab) : go(k_live_reduce_units<true>, tab);
    else q.term() ? go(k_live_reduce<false>) : go(k_live_reduce<true>);
}
// A Termination verdict as mc_live_info: `violating` components without a Done state, the least at first_root; size: at an id, the
// states of the component (the refined sizes after a refinement).  Ends the check.
int StateGraph::live_termination(uint64_t violating, uint32_t first_root, const uint32_t *size, std::chrono::steady_clock::time_point started, mc_live_info *out) {
    mc_live_info &li = lv.last.linfo;
    memset(&li, 0, sizeof li);
    li.violated = violating ? 1 : 0;
    li.fair_components = violating;
    if (violating) {
        uint32_t sz = 0;
        HIP_TRY(hipMemcpy(&sz, size + first_root, sizeof sz, hipMemcpyDeviceToHost));
        li.root = first_root;
        li.root_size = sz;
    }
    li.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - started).count();
    lv.last.checked = true;
    *out = li;
    return MC_OK;
}
// The weak entries: per state the masks, per component the rule, once.  Termination judges the full graph's components; a property is one
// (M, S, T) check over lv.pred: the components of G[M] (kept per mask), the rule per component, then the reach pass and the witness.
int StateGraph::live_single(const LiveQuery &q, hipStream_t stream, std::chrono::steady_clock::time_point started, mc_live_info *lout, mc_live_check_info *cout) {
    const uint64_t n = info.states;
    const bool term = q.term();
    const LiveCheck ck = term ? LiveCheck{} : LiveCheck{q.kind, q.p, q.q};
    int rc;
    uint32_t builds = 0;
    // ---- the components of G[M]: the full graph's for Termination and <>[]P, else one build per predicate that masks
    if (!term && (rc = live_mask_components(q.kind, q.q, stream, &lv.last.mask, &builds))) return rc;
    const Live::Masked *mask = lv.last.mask;
    const uint32_t *scc = mask ? mask->scc.p : lv.scc.p, *size = mask ? mask->size.p : lv.size.p, *pred = term ? nullptr : lv.pred.p;
    DevBuf<LiveCounters> d_lc;
    if ((rc = live_arrays(q))) return rc;
    if ((rc = graph_alloc(d_lc, 1, "the counters", q.call))) return rc;
    uint32_t *dist = term ? nullptr : lv.dist.p;
    LiveCounters lc;
    memset(&lc, 0, sizeof lc);
    lc.first_root = ~0u;
    HIP_TRY(hipMemcpyAsync(d_lc, &lc, sizeof lc, hipMemcpyHostToDevice, stream));
    if ((rc = live_clear(q, stream))) return rc;
    live_reduce(q, stream, scc, size, ck);
    auto verdict = [&](auto kernel) {
        live_launch(stream, kernel, n, scc, size, (const unsigned long long *)lv.taken.p, (const unsigned long long *)lv.disabled.p,
                    (const unsigned *)lv.done.p, q.all, q.weak, d_lc.p, pred, ck, dist);
    };
    term ? verdict(k_live_verdict<false>) : verdict(k_live_verdict<true>);
    if (!term) live_launch(stream, k_live_reach_init, n, scc, pred, ck, lv.dist.p);
    HIP_TRY(hipGetLastError());
    if (!term) return live_reach_tail(q, scc, size, builds, d_lc.p, 0, stream, started, cout);
    HIP_TRY(hipMemcpyAsync(&lc, d_lc, sizeof lc, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return live_termination(lc.fair_components, lc.first_root, lv.size.p, started, lout);
}
// What a property check does once dist[] is 0 on the states of the violating components and LIVE_FAR elsewhere: the reach pass, the
// witness, the counters, and — when violated, on the host — the descent from the witness into a component (lv.last.descent), which
// fixes the component reported.  scc / size: the ids and sizes the descent's component is read from (a refinement: the refined ones;
// fair_components is then the caller's count, d_lc is not read).  Ends the check.
int StateGraph::live_reach_tail(const LiveQuery &q, const uint32_t *scc, const uint32_t *size, uint32_t builds, const LiveCounters *d_lc, uint64_t strong_final,
                                hipStream_t stream, std::chrono::steady_clock::time_point started, mc_live_check_info *out) {
    const uint64_t n = info.states;
    const LiveCheck ck{q.kind, q.p, q.q};
    const uint32_t *pred = lv.pred.p;
    DevBuf<LiveCheckCounters> d_cc;
    DevBuf<unsigned> flag;
    int rc;
    if ((rc = graph_alloc(d_cc, 1, "the counters", "mc_engine_liveness_check"))) return rc;
    if ((rc = graph_alloc(flag, 1, "the fixed-point flag", "mc_engine_liveness_check"))) return rc;
    LiveCounters lc;
    memset(&lc, 0, sizeof lc);
    LiveCheckCounters cc;
    memset(&cc, 0, sizeof cc);
    cc.witness = ~0u;
    HIP_TRY(hipMemcpyAsync(d_cc, &cc, sizeof cc, hipMemcpyHostToDevice, stream));
    uint32_t sweeps = 0;
    if (n && (rc = live_fixed_point(stream, flag.p, sweeps, [&] { live_launch(stream, k_live_reach, n, (const uint64_t *)offsets.p, (const uint32_t *)dst.p, pred, ck, lv.dist.p, flag.p); },
                                    n + SCC_BATCH, "mc_engine_liveness_check: the reach pass")))
        return rc;
    live_launch(stream, k_live_witness, n, pred, ck, (const uint32_t *)lv.dist.p, (uint64_t)info.init_states, d_cc.p);
    HIP_TRY(hipGetLastError());
    if (d_lc) HIP_TRY(hipMemcpyAsync(&lc, d_lc, sizeof lc, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&cc, d_cc, sizeof cc, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    memset(out, 0, sizeof *out);
    out->violated = cc.bad_starts ? 1 : 0;
    out->sweeps = sweeps;
    out->fair_components = d_lc ? lc.fair_components : strong_final;
    out->mask_states = cc.mask_states;
    out->bad_starts = cc.bad_starts;
    out->scc_builds = builds;
    std::vector<uint32_t> &descent = lv.last.descent;
    if (out->violated) {
        // from the witness along strictly falling dist inside M, the least such successor each time
        std::vector<uint64_t> off((size_t)n + 1);
        std::vector<uint32_t> d((size_t)info.edges), dist((size_t)n);
        HIP_TRY(hipMemcpy(off.data(), offsets.p, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(dist.data(), lv.dist.p, dist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (info.edges) HIP_TRY(hipMemcpy(d.data(), dst.p, d.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint32_t cur = cc.witness;
        descent.push_back(cur);
        while (dist[cur] != 0) {
            uint32_t best = ~0u;
            for (uint64_t k = off[cur]; k < off[cur + 1]; ++k) {
                const uint32_t t = d[(size_t)k];
                if (t < n && t != cur && dist[t] != LIVE_FAR && dist[t] + 1 == dist[cur] && t < best) best = t;   // (a dist at all: the state is in M)
            }
            if (best == ~0u) { set_error("mc_engine_liveness_check: state " + std::to_string(cur) + " has a distance and no successor one step nearer"); return MC_ESTATE; }
            descent.push_back(best);
            cur = best;
        }
        uint32_t root = 0, sz = 0;
        HIP_TRY(hipMemcpy(&root, scc + cur, sizeof root, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&sz, size + root, sizeof sz, hipMemcpyDeviceToHost));
        out->witness = cc.witness;
        out->root = root;
        out->root_size = sz;
    }
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - started).count();
    mc_live_info &li = lv.last.linfo;
    memset(&li, 0, sizeof li);
    li.violated = out->violated;
    li.fair_components = out->fair_components;
    li.root = out->root;
    li.root_size = out->root_size;
    li.seconds = out->seconds;
    lv.last.checked = true;
    return MC_OK;
}
// The strong and unit entries: a check under strong fairness of the processes of q.strong, liveness.h's refinement,
// one round per loop.  Termination: M = all, T = not Done (lout), else the (M, S, T) check of live_single (cout).  Round 1 runs on the
// components a weak check of the same M uses — lv.scc, or the mask's build, made and kept here as live_single does —, later rounds on
// builds of the open subgraph into lv.wscc / lv.wsize; nothing a weak check reads is written.  One blocking read per round beside the
// build's.  q.fu: lv.unit holds the edges' UNITS, the masks are masks of fairness conjuncts, and the table-driven
// twins of the three kernels that read the edges are launched.
int StateGraph::live_refined(const LiveQuery &q, hipStream_t stream, std::chrono::steady_clock::time_point started, mc_live_info *lout, mc_live_check_info *cout,
                             mc_live_strong_info *sout) {
    const uint64_t n = info.states, cells = n ? n : 1;
    const bool term = q.term(), units = q.fu != nullptr;
    const uint64_t all = q.all, weak = q.weak, strong = q.strong;
    const LiveCheck ck{term ? LIVE_STABLE : q.kind, q.p, q.q};   // (Termination: every state is in M; the target is the Done flag's, not a predicate's)
    int rc;
    uint32_t builds = 0;
    if (units) {
        lv.of_unit_host.assign(q.fu->of_unit, q.fu->of_unit + LIVE_UNIT_TAB);
        if ((rc = graph_alloc(lv.of_unit, LIVE_UNIT_TAB, "the units' conjuncts", q.call))) return rc;
        HIP_TRY(hipMemcpyAsync(lv.of_unit, lv.of_unit_host.data(), LIVE_UNIT_TAB * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    }
    const uint64_t *d_tab = lv.of_unit.p;
    const int8_t *edge_class = units ? lv.unit.p : lv.proc.p;
    if (!term && (rc = live_mask_components(q.kind, q.q, stream, &lv.last.mask, &builds))) return rc;
    const Live::Masked *mask = lv.last.mask;
    const uint32_t *pred = term ? nullptr : lv.pred.p;
    DevBuf<LiveStrongCounters> d_sc;
    if ((rc = live_arrays(q))) return rc;
    if ((rc = graph_alloc(d_sc, 1, "the counters", q.call))) return rc;
    uint32_t *dist = term ? nullptr : lv.dist.p;
    LiveStrongCounters sc;
    memset(&sc, 0, sizeof sc);
    sc.first_root = ~0u;
    HIP_TRY(hipMemcpyAsync(d_sc, &sc, sizeof sc, hipMemcpyHostToDevice, stream));
    if (!term) HIP_TRY(hipMemsetAsync(lv.dist, 0xff, cells * sizeof(uint32_t), stream));   // (LIVE_FAR; k_live_refine puts 0 on the final components)
    if (term) live_launch(stream, k_live_open_init<false>, n, pred, ck, lv.open.p, lv.fscc.p, lv.fsize.p);
    else live_launch(stream, k_live_open_init<true>, n, pred, ck, lv.open.p, lv.fscc.p, lv.fsize.p);
    const uint32_t *scc = mask ? mask->scc.p : lv.scc.p, *size = mask ? mask->size.p : lv.size.p;
    // the two other passes that read the edges: `tab` is the staged table of the _units twin, or nothing
    auto enabled = [&](auto kernel, auto... tab) {
        live_launch(stream, kernel, n, (const uint64_t *)offsets.p, (const uint32_t *)dst.p, edge_class, scc, size, (const uint8_t *)lv.open.p, lv.enabled.p, tab...);
    };
    auto refine = [&](auto kernel, auto... tab) {
        live_launch(stream, kernel, n, (const uint64_t *)offsets.p, (const uint32_t *)dst.p, edge_class, scc, size, (const unsigned long long *)lv.taken.p,
                    (const unsigned long long *)lv.disabled.p, (const unsigned *)lv.done.p, (const unsigned long long *)lv.enabled.p, all, weak, strong, term,
                    lv.open.p, lv.fscc.p, lv.fsize.p, dist, d_sc.p, tab...);
    };
    const uint32_t bound = live_strong_rounds(all, strong);
    uint32_t rounds = 0, strong_builds = 0;
    for (;;) {
        ++rounds;
        if ((rc = live_clear(q, stream))) return rc;
        HIP_TRY(hipMemsetAsync(&d_sc.p->open, 0, sizeof(unsigned), stream));
        live_reduce(q, stream, scc, size, ck);
        units ? enabled(k_live_enabled_units, d_tab) : enabled(k_live_enabled);
        live_launch(stream, k_live_classify, n, scc, size, (const uint8_t *)lv.open.p, (const unsigned long long *)lv.taken.p,
                    (const unsigned long long *)lv.disabled.p, (const unsigned *)lv.done.p, (const unsigned long long *)lv.enabled.p, all, weak, strong, term,
                    d_sc.p);
        units ? refine(k_live_refine_units, d_tab) : refine(k_live_refine);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&sc, d_sc, sizeof sc, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (!sc.open) break;
        if (rounds >= bound) {
            set_error(std::string(q.call) + ": the refinement did not converge after " + std::to_string(rounds) + " rounds (" + std::to_string(bound - 1) +
                      (units ? " strong conjuncts)" : " strongly fair processes)"));
            return MC_ESTATE;
        }
        mc_scc_info si;
        if ((rc = scc_components(n, stream, -1, lv.wscc, lv.wsize, si, lv.open.p))) return rc;
        ++strong_builds;
        scc = lv.wscc.p;
        size = lv.wsize.p;
    }
    memset(sout, 0, sizeof *sout);
    sout->rounds = rounds;
    sout->scc_builds = strong_builds;
    sout->closed_states = sc.closed;
    sout->final_components = sc.final_components;
    if (term) {
        if ((rc = live_termination(sc.final_components, sc.first_root, lv.fsize.p, started, lout))) return rc;
        sout->seconds = lout->seconds;
        return MC_OK;
    }
    if ((rc = live_reach_tail(q, lv.fscc.p, lv.fsize.p, builds, nullptr, sc.final_components, stream, started, cout))) return rc;
    sout->seconds = cout->seconds;
    return MC_OK;
}
// The counterexample of the last mc_engine_liveness, built on the host from the arrays (deterministic given them).
// prefix: from an initial state to the chosen component's id (its least state) — after a property check: to the witness, and on along
// lv.last.descent to the first state of the component —, one BFS level back per step along the transpose: the
// least source in the previous level (level boundaries: level_start).  cycle: a closed walk inside the component that starts at
// that state and, for every weakly fair process, takes a real step of it or passes a state where it is disabled; the last entry has an
// edge back to the first.  Empty = the behaviour stutters in the prefix's last state for ever.  After a check by units (DESIGN section
// 21) "process" reads "conjunct": a step of it is an edge whose unit belongs to it.
int StateGraph::live_trace(const std::vector<uint64_t> &level_start, uint32_t *prefix_out, size_t *nprefix_inout, uint32_t *cycle_out, size_t *ncycle_inout) {
    if (!built || !lv.last.checked) { set_error("mc_engine_liveness_trace: no liveness check (mc_engine_liveness runs it; the next search releases it)"); return MC_ESTATE; }
    if (!lv.last.linfo.violated) { set_error("mc_engine_liveness_trace: the property holds: there is no counterexample"); return MC_ESTATE; }
    HIP_TRY(hipSetDevice(device));
    const uint64_t n = info.states, edges = info.edges;
    const uint32_t root = (uint32_t)lv.last.linfo.root;
    const bool prop = lv.last.kind >= 0 && !lv.last.descent.empty();
    const uint32_t target = prop ? lv.last.descent.front() : root;   // where the way back to an initial state starts
    // ---- prefix
    std::vector<uint32_t> prefix{target};
    auto level_of = [&](uint32_t x) { return (size_t)(std::upper_bound(level_start.begin(), level_start.end(), (uint64_t)x) - level_start.begin()) - 1; };
    for (uint32_t cur = target; level_of(cur) > 0;) {
        const size_t L = level_of(cur);
        uint64_t row[2];
        HIP_TRY(hipMemcpy(row, lv.toff.p + cur, sizeof row, hipMemcpyDeviceToHost));
        std::vector<uint32_t> src((size_t)(row[1] - row[0]));
        if (!src.empty()) HIP_TRY(hipMemcpy(src.data(), lv.tsrc.p + row[0], src.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint32_t best = ~0u;
        for (uint32_t u : src) if (u >= level_start[L - 1] && u < level_start[L] && u < best) best = u;
        if (best == ~0u) { set_error("mc_engine_liveness_trace: state " + std::to_string(cur) + " has no in-edge from the level before its own"); return MC_ESTATE; }
        prefix.push_back(best);
        cur = best;
    }
    std::reverse(prefix.begin(), prefix.end());
    if (prop) prefix.insert(prefix.end(), lv.last.descent.begin() + 1, lv.last.descent.end());
    const uint32_t entry = prefix.back();   // where the behaviour enters the component: the cycle starts and ends here
    // ---- cycle
    std::vector<uint64_t> off((size_t)n + 1);
    std::vector<uint32_t> dst((size_t)edges), scc((size_t)n);
    std::vector<int8_t> proc((size_t)edges);
    HIP_TRY(hipMemcpy(off.data(), offsets.p, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(scc.data(), lv.last.refined ? lv.fscc.p : prop && lv.last.mask ? lv.last.mask->scc.p : lv.scc.p, scc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (edges) {
        HIP_TRY(hipMemcpy(dst.data(), this->dst.p, dst.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(proc.data(), lv.last.units ? lv.unit.p : lv.proc.p, proc.size() * sizeof(int8_t), hipMemcpyDeviceToHost));
    }
    const uint64_t *tab = lv.last.units ? lv.of_unit_host.data() : nullptr;
    auto counts_for = [&](int8_t pr, int p) { return tab ? (live_conjuncts(tab, pr) >> p & 1) != 0 : pr == p; };   // is an edge of pr a step of p
    std::vector<uint32_t> members;
    for (uint64_t v = 0; v < n; ++v) if (scc[(size_t)v] == root) members.push_back((uint32_t)v);
    std::vector<uint32_t> par((size_t)n, ~0u);
    std::vector<uint32_t> cycle{entry};   // the walk so far; its last entry is where it stands
    // breadth-first inside the component, rows in index order; appends the states after `from` up to `to`
    auto go = [&](uint32_t to) {
        const uint32_t from = cycle.back();
        if (from == to) return true;
        for (uint32_t m : members) par[m] = ~0u;
        std::vector<uint32_t> q{from};
        par[from] = from;
        for (size_t h = 0; h < q.size() && par[to] == ~0u; ++h)
            for (uint64_t k = off[q[h]]; k < off[q[h] + 1]; ++k) {
                const uint32_t d = dst[(size_t)k];
                if (scc[d] == root && par[d] == ~0u) { par[d] = q[h]; q.push_back(d); }
            }
        if (par[to] == ~0u) return false;
        std::vector<uint32_t> path;
        for (uint32_t x = to; x != from; x = par[x]) path.push_back(x);
        cycle.insert(cycle.end(), path.rbegin(), path.rend());
        return true;
    };
    bool ok = true;
    for (int p = 0; p < 64 && ok; ++p) {
        if (!((lv.last.fair | lv.last.strong) >> p & 1)) continue;
        const bool sf = lv.last.strong >> p & 1;   // strongly fair: taken inside, or — the refinement saw to it — disabled everywhere in the component
        bool found = false;
        for (size_t mi = 0; mi < members.size() && !found; ++mi) {   // a real step of p inside the component: the first in index order
            const uint32_t u = members[mi];
            for (uint64_t k = off[u]; k < off[u + 1] && !found; ++k)
                if (counts_for(proc[(size_t)k], p) && live_real_step(proc[(size_t)k], u, dst[(size_t)k]) && scc[dst[(size_t)k]] == root) {
                    found = true;
                    ok = go(u);
                    cycle.push_back(dst[(size_t)k]);
                }
        }
        if (sf) found = true;
        for (size_t mi = 0; mi < members.size() && !found; ++mi) {   // else a state where p is disabled
            const uint32_t u = members[mi];
            uint64_t en = 0, tk = 0;
            bool dn = false;
            if (tab) live_state_units(u, dst.data() + off[u], proc.data() + off[u], off[u + 1] - off[u], scc.data(), tab, &en, &tk, &dn);
            else live_state(u, dst.data() + off[u], proc.data() + off[u], off[u + 1] - off[u], scc.data(), &en, &tk, &dn);
            if (!(en >> p & 1)) { found = true; ok = go(u); }
        }
        if (!found) ok = false;
    }
    if (ok && prop && lv.last.kind == LIVE_STABLE) {   // <>[]P: the walk passes a ~P state, the component's least
        std::vector<uint32_t> bits((size_t)n);
        HIP_TRY(hipMemcpy(bits.data(), lv.pred.p, bits.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        const LiveCheck ck{lv.last.kind, lv.last.p, lv.last.q};
        bool found = false;
        for (size_t mi = 0; mi < members.size() && !found; ++mi)
            if (live_in_target(ck, bits[members[mi]])) { found = true; ok = go(members[mi]); }
        if (!found) ok = false;
    }
    if (ok) ok = go(entry);
    if (!ok) { set_error("mc_engine_liveness_trace: the chosen component is not fair or not connected (the arrays disagree with the verdict)"); return MC_ESTATE; }
    cycle.pop_back();   // (the walk ended on `entry` again: the closing edge is implied; a walk that never moved leaves nothing)
    if (prefix.size() > *nprefix_inout || cycle.size() > *ncycle_inout || !prefix_out || (!cycle.empty() && !cycle_out)) {
        *nprefix_inout = prefix.size();
        *ncycle_inout = cycle.size();
        set_error("mc_engine_liveness_trace: buffers too small (" + std::to_string(prefix.size()) + " + " + std::to_string(cycle.size()) + " states)");
        return MC_EBADCFG;
    }
    memcpy(prefix_out, prefix.data(), prefix.size() * sizeof(uint32_t));
    if (!cycle.empty()) memcpy(cycle_out, cycle.data(), cycle.size() * sizeof(uint32_t));
    *nprefix_inout = prefix.size();
    *ncycle_inout = cycle.size();
    return MC_OK;
}

}  // namespace mc
