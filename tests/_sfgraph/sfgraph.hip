// sfgraph.hip — the test-only driver of mc::StateGraph for the checks under strong fairness (tests/sfgraph.py, tests/sfrandgraph.py):
// tests/_sgraph/sgraph.hip's driver, included whole — its handle, its uploads, its preparation in the engine's order, its sg_* entries —
// and two entries more.  No kernel lives here and nothing of libtlamc.so is linked: what runs on the device is engine_live.h alone.
#include "../_sgraph/sgraph.hip"

extern "C" {

// engine.hip's liveness_strong / liveness_check_strong: the masks' conditions, the weak twins' preparation, then the call
static int sf_masks(uint64_t all, uint64_t weak, uint64_t strong, const char *call) {
    if ((weak | strong) & ~all) { mc::set_error(std::string(call) + ": a fairness mask names a process instance the program does not have"); return MC_EBADCFG; }
    if (weak & strong) { mc::set_error(std::string(call) + ": the weak and the strong mask overlap"); return MC_EBADCFG; }
    return MC_OK;
}
int sf_live_strong(void *h, uint64_t all, uint64_t weak, uint64_t strong, mc_live_info *out, mc_live_strong_info *sout) {
    Sg &s = *(Sg *)h;
    memset(out, 0, sizeof *out);
    memset(sout, 0, sizeof *sout);
    if (int rc = sf_masks(all, weak, strong, "sf_live_strong")) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (int rc = prepare(s, true, false, "sf_live_strong")) return rc;
    return s.g.live_check_strong(all, weak, strong, -1, -1, -1, s.stream, t0, out, nullptr, sout);
}
int sf_live_check_strong(void *h, uint64_t all, uint64_t weak, uint64_t strong, int kind, int p, int q, mc_live_check_info *out, mc_live_strong_info *sout) {
    Sg &s = *(Sg *)h;
    memset(out, 0, sizeof *out);
    memset(sout, 0, sizeof *sout);
    if (int rc = sf_masks(all, weak, strong, "sf_live_check_strong")) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (int rc = prepare(s, false, true, "sf_live_check_strong")) return rc;
    return s.g.live_check_strong(all, weak, strong, kind, p, q, s.stream, t0, nullptr, out, sout);
}

}  // extern "C"
