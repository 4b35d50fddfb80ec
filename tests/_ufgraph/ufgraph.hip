// ufgraph.hip — the test-only driver of mc::StateGraph for the checks label by label (tests/ufgraph.py, tests/ufrandgraph.py):
// tests/_sfgraph/sfgraph.hip's driver, included whole — tests/_sgraph/sgraph.hip's handle, uploads and preparation, the sg_* and sf_*
// entries —, the edges' units beside the edges' processes, and two entries more.  No kernel lives here and nothing of libtlamc.so is
// linked: what runs on the device is engine_live.h alone.
#include "../_sfgraph/sfgraph.hip"

#include <map>

namespace {
std::map<void *, std::vector<int8_t>> g_units;   // per handle: the edges' units (uf_set_units), uploaded where the engine enqueues k_live_unit
}

extern "C" {

int uf_set_units(void *h, const int8_t *unit) {
    Sg &s = *(Sg *)h;
    for (uint64_t k = 0; k < s.g.info.edges; ++k)
        if (unit[k] < -1) { mc::set_error("uf_set_units: edge " + std::to_string(k) + " has no unit in -1 .. 126"); return MC_EBADCFG; }
    g_units[h].assign(unit, unit + s.g.info.edges);
    return MC_OK;
}
void uf_destroy(void *h) { g_units.erase(h); sg_destroy(h); }
// what sgraph.hip's check does more for a check by units: the edges' units beside the edges' processes (proc[] stays what a
// process-level check reads).  The query is refused first, and by the product (live_query.h): the look at the units reads a table
// that is in range.
static int uf_units(Sg &s, const mc::LiveQuery &q) {
    if (int rc = mc::live_query_check(q, mc::LIVE_MAX_PREDS)) return rc;
    auto it = g_units.find((void *)&s);
    if (it == g_units.end()) { mc::set_error(std::string(q.call) + ": the graph has no units (uf_set_units)"); return MC_EBADCFG; }
    for (int8_t u : it->second)
        if (u >= q.fu->nunits) { mc::set_error(std::string(q.call) + ": an edge's unit is beyond nunits"); return MC_EBADCFG; }
    if (!s.g.lv.unit_built) {
        if (int rc = upload(s.g.lv.unit, it->second.data(), s.g.info.edges, "the edges' units")) return rc;
        s.g.lv.unit_built = true;
    }
    return MC_OK;
}
int uf_live_units(void *h, const mc_fair_units *fu, mc_live_info *out, mc_live_strong_info *sout) {
    return check(*(Sg *)h, mc::live_query_units("uf_live_units", fu, -1, -1, -1), out, nullptr, sout, uf_units);
}
int uf_live_check_units(void *h, const mc_fair_units *fu, int kind, int p, int q, mc_live_check_info *out, mc_live_strong_info *sout) {
    return check(*(Sg *)h, mc::live_query_units("uf_live_check_units", fu, kind, p, q), nullptr, out, sout, uf_units);
}

}  // extern "C"
