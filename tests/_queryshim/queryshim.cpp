// queryshim.cpp — a test-only door to tla_rust_amd/csrc/live_query.h (tests/test_live_query_host.py): the one validation of a liveness
// query and its normalisation, built with g++ and no HIP.  Nothing is decided here: a row of the test's table becomes a LiveQuery, and
// what live_query_error and live_query_normalised say about it is handed back.
#include "live_query.h"   // -I the product's csrc

#include <stdio.h>

extern "C" {

// fu null: a process-level query over all / weak / strong; else the query of a check label by label, as the engine's entries make it
// (live_query_units: the masks are the table's).  Returns 1 when refused, with the reason in msg; p_out / q_out: the normalised indices.
int queryshim_check(int refine, uint64_t all, uint64_t weak, uint64_t strong, const mc_fair_units *fu, int kind, int p, int q, int npred, char *msg, size_t cap,
                    int *p_out, int *q_out) {
    const mc::LiveQuery query = fu ? mc::live_query_units("shim", fu, kind, p, q) : mc::LiveQuery{"shim", all, weak, strong, nullptr, kind, p, q, refine != 0};
    const std::string why = mc::live_query_error(query, npred);
    snprintf(msg, cap, "%s", why.c_str());
    const mc::LiveQuery norm = mc::live_query_normalised(query);
    *p_out = norm.p;
    *q_out = norm.q;
    return why.empty() ? 0 : 1;
}

}  // extern "C"
