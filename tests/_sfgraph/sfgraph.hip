// sfgraph.hip — the test-only driver of mc::StateGraph for the checks under strong fairness (tests/sfgraph.py, tests/sfrandgraph.py):
// tests/_sgraph/sgraph.hip's driver, included whole — its handle, its uploads, its preparation in the engine's order, its sg_* entries —
// and two entries more.  No kernel lives here and nothing of libtlamc.so is linked: what runs on the device is engine_live.h alone.
#include "../_sgraph/sgraph.hip"

extern "C" {

int sf_live_strong(void *h, uint64_t all, uint64_t weak, uint64_t strong, mc_live_info *out, mc_live_strong_info *sout) {
    return check(*(Sg *)h, mc::LiveQuery{"sf_live_strong", all, weak, strong, nullptr, -1, -1, -1, true}, out, nullptr, sout);
}
int sf_live_check_strong(void *h, uint64_t all, uint64_t weak, uint64_t strong, int kind, int p, int q, mc_live_check_info *out, mc_live_strong_info *sout) {
    return check(*(Sg *)h, mc::LiveQuery{"sf_live_check_strong", all, weak, strong, nullptr, kind, p, q, true}, nullptr, out, sout);
}

}  // extern "C"
