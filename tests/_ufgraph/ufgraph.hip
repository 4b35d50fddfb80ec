// ufgraph.hip — the test-only driver of mc::StateGraph for the checks label by label (tests/ufgraph.py, tests/ufrandgraph.py):
// tests/_sfgraph/sfgraph.hip's driver, included whole — tests/_sgraph/sgraph.hip's handle, uploads and preparation, the sg_* and sf_*
// entries —, the edges' units beside the edges' processes, and two entries more.  No kernel lives here and nothing of libtlamc.so is
// linked: what runs on the device is engine_live.h alone.
#include "../_sfgraph/sfgraph.hip"

#include <map>

#include "liveness.h"

namespace {
std::map<void *, std::vector<int8_t>> g_units;   // per handle: the edges' units (uf_set_units), uploaded where the engine enqueues k_live_unit
}

extern "C" {

// engine.hip's units_prepare: the table's conditions
static int uf_table(const mc_fair_units *fu, const char *call) {
    const std::string c(call);
    if (fu->nunits < 0 || fu->nunits > mc::LIVE_MAX_UNITS) { mc::set_error(c + ": " + std::to_string(fu->nunits) + " units (at most 127)"); return MC_EBADCFG; }
    if (fu->nconj < 0 || fu->nconj > mc::LIVE_MAX_CONJ) { mc::set_error(c + ": " + std::to_string(fu->nconj) + " conjuncts (at most 64)"); return MC_EBADCFG; }
    const uint64_t all = mc::live_all_conjuncts(fu->nconj);
    if ((fu->weak_mask | fu->strong_mask) & ~all) { mc::set_error(c + ": a fairness mask names a conjunct beyond nconj"); return MC_EBADCFG; }
    if (fu->weak_mask & fu->strong_mask) { mc::set_error(c + ": the weak and the strong mask overlap (a conjunct is WF or SF)"); return MC_EBADCFG; }
    for (int u = 0; u < mc::LIVE_UNIT_TAB; ++u)
        if (fu->of_unit[u] & (u < fu->nunits ? ~all : ~0ull)) { mc::set_error(c + ": of_unit[" + std::to_string(u) + "] names a conjunct it cannot"); return MC_EBADCFG; }
    return MC_OK;
}
int uf_set_units(void *h, const int8_t *unit) {
    Sg &s = *(Sg *)h;
    for (uint64_t k = 0; k < s.g.info.edges; ++k)
        if (unit[k] < -1) { mc::set_error("uf_set_units: edge " + std::to_string(k) + " has no unit in -1 .. 126"); return MC_EBADCFG; }
    g_units[h].assign(unit, unit + s.g.info.edges);
    return MC_OK;
}
void uf_destroy(void *h) { g_units.erase(h); sg_destroy(h); }
static int uf_prepare(Sg &s, void *h, const mc_fair_units *fu, bool want_pred, const char *call) {
    if (int rc = uf_table(fu, call)) return rc;
    auto it = g_units.find(h);
    if (it == g_units.end()) { mc::set_error(std::string(call) + ": the graph has no units (uf_set_units)"); return MC_EBADCFG; }
    for (int8_t u : it->second)
        if (u >= fu->nunits) { mc::set_error(std::string(call) + ": an edge's unit is beyond nunits"); return MC_EBADCFG; }
    if (int rc = prepare(s, false, want_pred, call)) return rc;   // (the components; proc[] stays what a process-level check reads)
    if (!s.g.lv.unit_built) {
        if (int rc = upload(s.g.lv.unit, it->second.data(), s.g.info.edges, "the edges' units")) return rc;
        s.g.lv.unit_built = true;
    }
    return MC_OK;
}
int uf_live_units(void *h, const mc_fair_units *fu, mc_live_info *out, mc_live_strong_info *sout) {
    Sg &s = *(Sg *)h;
    memset(out, 0, sizeof *out);
    memset(sout, 0, sizeof *sout);
    const auto t0 = std::chrono::steady_clock::now();
    if (int rc = uf_prepare(s, h, fu, false, "uf_live_units")) return rc;
    return s.g.live_check_strong(mc::live_all_conjuncts(fu->nconj), fu->weak_mask, fu->strong_mask, -1, -1, -1, s.stream, t0, out, nullptr, sout, fu->of_unit);
}
int uf_live_check_units(void *h, const mc_fair_units *fu, int kind, int p, int q, mc_live_check_info *out, mc_live_strong_info *sout) {
    Sg &s = *(Sg *)h;
    memset(out, 0, sizeof *out);
    memset(sout, 0, sizeof *sout);
    const auto t0 = std::chrono::steady_clock::now();
    if (int rc = uf_prepare(s, h, fu, true, "uf_live_check_units")) return rc;
    return s.g.live_check_strong(mc::live_all_conjuncts(fu->nconj), fu->weak_mask, fu->strong_mask, kind, p, q, s.stream, t0, nullptr, out, sout, fu->of_unit);
}

}  // extern "C"
