// packshim.cpp — host build of spec_raft.h and spec_raft_packed.h side by side (no HIP): SpecRaft<3> and SpecRaftPacked<3> run in
// lockstep over a model's whole graph (bfs) or over fixed-seed random walks (walk), every slot of every state they meet.  What is
// compared per (state, slot) and what is counted is in check_state; the result is one JSON object on stdout, the first mismatch
// ends the run with a message on stderr and exit status 1.  tests/test_raft_packed_host.py builds and runs it.
//
//   packshim bfs   P0 P1 ...           the complete graph of raft with the device parameters P (breadth first, exact fingerprints' dedup)
//   packshim walk  SEED N DEPTH P0 ... N random walks of at most DEPTH steps
//   packshim script P0 P1 ...          scripted behaviours (run_script): second elections by servers that hold a log
//   packshim packable                  packable() of the three-server lowering at every log width the test names
//   packshim field                     lb = 6: entry (2, 2) of voterLog set to all ones, through import_row and through the writer
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <unordered_set>
#include <vector>

#include "../../tla_rust_amd/csrc/spec_raft_packed.h"

using namespace mc;
using B = SpecRaft<3>;
using P = SpecRaftPacked<3>;
static constexpr int NS = 3;

[[noreturn]] static void fail(const std::string &what) {
    fprintf(stderr, "packshim: MISMATCH: %s\n", what.c_str());
    exit(1);
}

struct Coverage {
    unsigned long long cls[B::NCLS] = {}, vl[NS][NS] = {}, two_elections = 0, clear_between = 0, clear_any = 0, vset = 0, eadd = 0;
    unsigned long long states = 0, pairs = 0, generated = 0, successors = 0, ambiguous_fp = 0;
};

static RaftParams make(const std::vector<int64_t> &p) {
    RaftParams prm;
    if (B::make_params(p.data(), (unsigned)p.size(), prm)) { fprintf(stderr, "packshim: bad parameters\n"); exit(2); }
    if (!P::packable(prm)) { fprintf(stderr, "packshim: the parameters do not pack\n"); exit(2); }
    return prm;
}

static void expect_row(const RaftParams &prm, const uint64_t *packed, const uint64_t *base, const char *who, int slot) {
    uint64_t pub[B::MAX_WORDS];
    P::export_row(prm, packed, pub);
    if (memcmp(pub, base, sizeof(uint64_t) * B::words(prm)) != 0) {
        std::string s = std::string(who) + ": export_row(packed successor) differs from the base successor, slot " + std::to_string(slot) + ", words";
        for (int w = 0; w < B::words(prm); w++) if (pub[w] != base[w]) s += " " + std::to_string(w);
        fail(s);
    }
    uint64_t back[P::MAX_WORDS];
    P::import_row(prm, pub, back);
    if (memcmp(back, packed, sizeof(uint64_t) * P::words(prm)) != 0) fail(std::string(who) + ": import_row(export_row(row)) is not the row");
}

template <int FAM>
static void check_pair(const RaftParams &prm, const B::Summary &qb, const P::Summary &qp, const uint64_t *sb, const uint64_t *sp, int slot) {
    uint64_t fb = 0, fp = 0;
    const unsigned stb = B::eval_pair<FAM>(prm, qb, CWordRef{sb, 1}, slot, fb);
    const unsigned stp = P::eval_pair<FAM>(prm, qp, CWordRef{sp, 1}, slot, fp);
    if (stb != stp || (stb && fb != fp)) fail("eval_pair: status or fingerprint, slot " + std::to_string(slot));
}

// every slot of one state; the stored successors (base rows) are appended to `succ`
static void check_state(const RaftParams &prm, const uint64_t *sb, Coverage &cv, std::vector<uint64_t> *succ, std::vector<int> *succ_slot = nullptr) {
    const int WB = B::words(prm), WP = P::words(prm);
    uint64_t sp[P::MAX_WORDS];
    P::import_row(prm, sb, sp);
    expect_row(prm, sp, sb, "state", -1);
    const CWordRef rb{sb, 1}, rp{sp, 1};
    if (P::fp_of(prm, rp) != B::fp_of(prm, rb) || P::fp_recompute(prm, rp) != B::fp_recompute(prm, rb)) fail("fingerprint of a state");
    B::Local lb, lp, eb, ep;
    B::Guards gb, gp;
    B::load(prm, rb, lb);
    P::load(prm, rp, lp);
    B::load_expand(prm, rb, eb, gb);
    P::load_expand(prm, rp, ep, gp);
    B::Summary qb, qp;
    B::summarize(eb, qb);
    P::summarize(ep, qp);
    if (memcmp(&qb, &qp, sizeof qb) != 0 || gb.fixed != gp.fixed || gb.fixed_hi != gp.fixed_hi || gb.infl != gp.infl) fail("load_expand: Summary or Guards");
    {
        B::Summary q1, q2;
        B::summarize(lb, q1);
        P::summarize(lp, q2);
        if (memcmp(&q1, &q2, sizeof q1) != 0 || memcmp(&q1, &qb, sizeof q1) != 0) fail("load: Summary");
    }
    int lo_b, n_b, lo_p, n_p;
    B::stage_range(prm, rb, lo_b, n_b);
    P::stage_range(prm, rp, lo_p, n_p);
    if (n_b != n_p || lo_p != P::P_MSG0) fail("stage_range");
    for (int k = 0; k < lb.nm; k++) if (B::rd_msg(rb, k) != P::rd_msg(rp, k)) fail("rd_msg");
    cv.states++;
    const uint64_t g = B::rd_glob(rb);
    if (B::g_ne(g) >= 2) cv.two_elections++;
    for (int i = 0; i < NS; i++)
        for (int j = 0; j < NS; j++) if (B::vl_get(sb[B::W_VL(i)], j, prm)) cv.vl[i][j]++;
    for (int i = 0; i < NS; i++) {   // the dense pairs: the packed class inherits eval_dense, which must agree with eval through the view
        unsigned stR, stT;
        uint64_t fR = 0, fT = 0, f = 0;
        P::eval_dense(prm, ep, rp, i, stR, fR, stT, fT);
        B::Local l2 = lp;
        const unsigned s1 = P::eval(prm, l2, rp, P::dense_slot(i, 0), f);
        if (s1 != stR || (s1 && !(s1 & (ST_OUT_OF_MODEL | ST_OVERFLOW)) && f != fR)) fail("eval_dense: Restart");
        const unsigned s2 = P::eval(prm, l2, rp, P::dense_slot(i, 1), f);
        if (s2 != stT || (s2 && !(s2 & (ST_OUT_OF_MODEL | ST_OVERFLOW)) && f != fT)) fail("eval_dense: Timeout");
    }
    const int ns = B::nslots(prm, lb);
    if (ns != P::nslots(prm, lp)) fail("nslots");
    std::vector<uint64_t> ob(WB), op(P::MAX_WORDS);
    for (int slot = 0; slot < ns; slot++) {
        cv.pairs++;
        uint64_t fb = 0, fp = 0;
        const unsigned stb = B::eval(prm, lb, rb, slot, fb);
        const unsigned stp = P::eval(prm, lp, rp, slot, fp);
        if (stb != stp) fail("status bits, slot " + std::to_string(slot));
        if (stb && fb != fp) fail("successor fingerprint, slot " + std::to_string(slot));
        if (slot >= B::FIX && B::message_generated_only(prm, lb, rb, slot) != P::message_generated_only(prm, lp, rp, slot)) fail("message_generated_only");
        if (slot >= B::DENSE_SLOTS && slot < B::FIX) {
            const int fam = B::fixed_family(slot);
            if (fam == B::F_REQVOTE) check_pair<B::F_REQVOTE>(prm, qb, qp, sb, sp, slot);
            else if (fam == B::F_APPEND) check_pair<B::F_APPEND>(prm, qb, qp, sb, sp, slot);
            else check_pair<B::F_MISC>(prm, qb, qp, sb, sp, slot);
        }
        if (B::action_of(prm, sb, slot) != P::action_of(prm, sp, slot)) fail("action_of");
        if (!(stb & ST_ENABLED)) continue;
        cv.generated++;
        cv.cls[B::slot_class(slot)]++;
        if (stb & ST_OVERFLOW) { fprintf(stderr, "packshim: a slot array of the row is full (capacities too small for this model)\n"); exit(2); }
        if (stb & (ST_OUT_OF_MODEL | ST_SPECERR)) continue;
        {   // what the action does to voterLog (the base's own Delta)
            B::Delta d;
            int action;
            B::compute(prm, lb, rb, slot, d, action);
            if (d.vmode == 2 && d.vlog) cv.vset++;
            if (d.eadd) cv.eadd++;
            if (d.vmode == 1 && d.ovl) {
                cv.clear_any++;
                bool between = true;   // the fields next to the cleared one hold something: a clear that reached too far would show
                if (d.srv > 0 && !sb[B::W_VL(d.srv - 1)]) between = false;
                if (d.srv < NS - 1 && !sb[B::W_VL(d.srv + 1)]) between = false;
                if (between) cv.clear_between++;
            }
        }
        // the three writers against the base's successor
        B::apply(prm, rb, slot, WordRef{ob.data(), 1});
        std::fill(op.begin(), op.end(), 0xdeadbeefdeadbeefull);
        P::apply(prm, rp, slot, WordRef{op.data(), 1});
        expect_row(prm, op.data(), ob.data(), "apply", slot);
        if (op[WP] != 0xdeadbeefdeadbeefull) fail("apply wrote past the row");
        std::fill(op.begin(), op.end(), 0xdeadbeefdeadbeefull);
        P::apply_known_fp(prm, rp, slot, fp, WordRef{op.data(), 1});
        if (stb & ST_SELFLOOP) { if (P::fp_of(prm, CWordRef{op.data(), 1}) != B::fp_of(prm, rb)) fail("self loop: not the parent's fingerprint"); }
        else expect_row(prm, op.data(), ob.data(), "apply_known_fp", slot);
        std::fill(op.begin(), op.end(), 0xdeadbeefdeadbeefull);
        P::apply_summary_patch(prm, qp, rp, slot, fp, WordRef{op.data(), 1});
        if (!(stb & ST_SELFLOOP)) expect_row(prm, op.data(), ob.data(), "apply_summary_patch", slot);
        if (op[WP] != 0xdeadbeefdeadbeefull) fail("apply_summary_patch wrote past the row");
        {   // the base's in-wave writer gives the base's row too (the two writers of spec_raft.h agree: what the packed one is held to)
            std::vector<uint64_t> o2(WB);
            B::apply_summary_patch(prm, qb, rb, slot, fb, WordRef{o2.data(), 1});
            if (!(stb & ST_SELFLOOP) && memcmp(o2.data(), ob.data(), sizeof(uint64_t) * WB) != 0) fail("base: apply_summary_patch differs from apply");
        }
        // the incremental fingerprint equals the full recomputation, in both layouts
        const CWordRef so{op.data(), 1};
        if (!(stb & ST_SELFLOOP)) {
            if (P::fp_recompute(prm, so) != op[P::P_FP]) fail("incremental fingerprint differs from the full recomputation (packed), slot " + std::to_string(slot));
            if (B::fp_recompute(prm, CWordRef{ob.data(), 1}) != ob[B::W_FP]) fail("incremental fingerprint differs from the full recomputation (base)");
            if (fp_nonzero(op[P::P_FP]) != fp) fail("eval's fingerprint is not the written row's");
            if (fp == fp_nonzero(0)) cv.ambiguous_fp++;
        }
        cv.successors++;
        if (succ && !(stb & ST_SELFLOOP)) {
            succ->insert(succ->end(), ob.begin(), ob.end());
            if (succ_slot) succ_slot->push_back(slot);
        }
    }
}

static void print_cov(const Coverage &cv) {
    printf("\"states\": %llu, \"pairs\": %llu, \"generated\": %llu, \"successors\": %llu, \"classes\": [", cv.states, cv.pairs, cv.generated, cv.successors);
    for (int c = 0; c < B::NCLS; c++) printf("%s%llu", c ? ", " : "", cv.cls[c]);
    printf("], \"voterlog\": [");
    for (int i = 0; i < NS; i++) for (int j = 0; j < NS; j++) printf("%s%llu", i || j ? ", " : "", cv.vl[i][j]);
    printf("], \"two_elections\": %llu, \"clear_any\": %llu, \"clear_between\": %llu, \"vset\": %llu, \"eadd\": %llu", cv.two_elections, cv.clear_any, cv.clear_between, cv.vset, cv.eadd);
}

static std::vector<int64_t> params_from(int argc, char **argv, int first) {
    std::vector<int64_t> p;
    for (int a = first; a < argc; a++) p.push_back(atoll(argv[a]));
    return p;
}

static int run_bfs(int argc, char **argv) {
    const RaftParams prm = make(params_from(argc, argv, 2));
    const int WB = B::words(prm);
    std::vector<uint64_t> frontier(WB), next, succ;
    B::init(prm, 0, WordRef{frontier.data(), 1});
    {
        uint64_t ip[P::MAX_WORDS], pub[B::MAX_WORDS];
        P::init(prm, 0, WordRef{ip, 1});
        P::export_row(prm, ip, pub);
        if (memcmp(pub, frontier.data(), sizeof(uint64_t) * WB) != 0) fail("init");
    }
    std::unordered_set<uint64_t> seen{B::fp_of(prm, CWordRef{frontier.data(), 1})};
    Coverage cv;
    std::vector<unsigned long long> levels;
    while (!frontier.empty()) {
        levels.push_back(frontier.size() / WB);
        next.clear();
        for (size_t k = 0; k < frontier.size(); k += WB) {
            succ.clear();
            check_state(prm, &frontier[k], cv, &succ);
            for (size_t q = 0; q < succ.size(); q += WB)
                if (seen.insert(B::fp_of(prm, CWordRef{&succ[q], 1})).second) next.insert(next.end(), succ.begin() + q, succ.begin() + q + WB);
        }
        frontier.swap(next);
    }
    printf("{\"mode\": \"bfs\", \"words\": [%d, %d], \"distinct\": %zu, \"levels\": [", WB, P::words(prm), seen.size());
    for (size_t k = 0; k < levels.size(); k++) printf("%s%llu", k ? ", " : "", levels[k]);
    printf("], ");
    print_cov(cv);
    printf("}\n");
    return 0;
}

static int run_walk(int argc, char **argv) {
    uint64_t rng = strtoull(argv[2], nullptr, 0) * 0x9e3779b97f4a7c15ull + 1;
    const int nwalks = atoi(argv[3]), depth = atoi(argv[4]);
    const RaftParams prm = make(params_from(argc, argv, 5));
    const int WB = B::words(prm);
    Coverage cv;
    std::vector<uint64_t> cur(WB), succ;
    std::vector<int> slots;
    // A uniform choice among the successors dies in Restart / Timeout (half of all successors, and MaxTerm is 3) long before a second
    // election: the walk weighs a successor by the class of its slot, rare kinds first.  (Weights of the WALK: every slot of every
    // state it visits is checked, whatever its weight.)
    static const unsigned weight[B::NCLS] = {1, 2, 6, 40, 40, 40, 24, 12, 1, 1};
    unsigned long long steps = 0;
    for (int wk = 0; wk < nwalks; wk++) {
        B::init(prm, 0, WordRef{cur.data(), 1});
        for (int t = 0; t < depth; t++) {
            succ.clear();
            slots.clear();
            check_state(prm, cur.data(), cv, &succ, &slots);
            if (succ.empty()) break;
            rng = fmix64(rng + 0x632be59bd9b4e019ull);
            unsigned long long total = 0;
            for (int s : slots) total += weight[B::slot_class(s)];
            unsigned long long r = rng % total;
            size_t pick = 0;
            while (r >= weight[B::slot_class(slots[pick])]) r -= weight[B::slot_class(slots[pick++])];
            memcpy(cur.data(), &succ[pick * WB], sizeof(uint64_t) * WB);
            steps++;
        }
    }
    printf("{\"mode\": \"walk\", \"words\": [%d, %d], \"steps\": %llu, ", WB, P::words(prm), steps);
    print_cov(cv);
    printf("}\n");
    return 0;
}

// Scripted behaviours: what no short random walk reaches — a second election by servers that hold a log — step by step.  Every state
// on the way gets the whole lockstep check.  A step that is not enabled (or leaves the model) ends the run with status 2: the script is
// wrong for the parameters, not the lowering.
struct Script {
    const RaftParams &prm;
    Coverage &cv;
    std::vector<uint64_t> cur, succ;
    std::vector<int> slots;
    int WB;
    Script(const RaftParams &p, Coverage &c) : prm(p), cv(c), cur(B::words(p)), WB(B::words(p)) { B::init(prm, 0, WordRef{cur.data(), 1}); look(); }
    void look() { succ.clear(); slots.clear(); check_state(prm, cur.data(), cv, &succ, &slots); }
    bool take(int slot) {
        for (size_t k = 0; k < slots.size(); k++)
            if (slots[k] == slot) { memcpy(cur.data(), &succ[k * WB], sizeof(uint64_t) * WB); look(); return true; }
        return false;
    }
    void must(int slot, const char *what) { if (!take(slot)) { fprintf(stderr, "packshim: script: %s (slot %d) is not a stored successor here\n", what, slot); exit(2); } }
    void restart(int i) { must(i, "Restart"); }
    void timeout(int i) { must(NS + i, "Timeout"); }
    void become_leader(int i) { must(2 * NS + NS * NS + i, "BecomeLeader"); }
    void client_request(int i) { must(3 * NS + NS * NS + i, "ClientRequest"); }
    void receive_all() {   // (UpdateTerm and the append of an entry leave the message in the bag: it is received again)
        for (int n = 0; n < 8; n++) {
            int slot = -1;
            for (int s : slots) if (s >= B::FIX && (s - B::FIX) % 3 == 0) { slot = s; break; }
            if (slot < 0) return;
            take(slot);
        }
    }
    void request_vote(int i, int j) { must(2 * NS + i * NS + j, "RequestVote"); receive_all(); }
    void append_entries(int i, int j) { must(5 * NS + NS * NS + i * NS + j, "AppendEntries"); receive_all(); }
    // leader L of term 2 by the votes of L and f, one client request, replicated to f (and to the third server)
    void leader_with_log(int L, int f, bool everywhere) {
        timeout(L);
        request_vote(L, L);
        request_vote(L, f);
        become_leader(L);
        client_request(L);
        append_entries(L, f);
        if (everywhere) append_entries(L, 3 - L - f);
    }
};

static int run_script(int argc, char **argv) {
    const RaftParams prm = make(params_from(argc, argv, 2));
    Coverage cv;
    // voterLog[i][j] holds a log: leader i, its entry replicated to j (to a third server where j = i), then i stands again in term 3 and j votes
    for (int i = 0; i < NS; i++)
        for (int j = 0; j < NS; j++) {
            Script s(prm, cv);
            s.leader_with_log(i, j != i ? j : (i + 1) % NS, false);
            s.restart(i);
            s.timeout(i);
            s.request_vote(i, j);
            if (!B::vl_get(s.cur[B::W_VL(i)], j, prm)) { fprintf(stderr, "packshim: script: voterLog[%d][%d] stayed empty\n", i, j); return 2; }
        }
    {   // two election records: term 2 and term 3, no client request in between
        Script s(prm, cv);
        s.timeout(0); s.request_vote(0, 0); s.request_vote(0, 1); s.become_leader(0);
        s.timeout(1); s.request_vote(1, 1); s.request_vote(1, 2); s.become_leader(1);
        if (B::g_ne(B::rd_glob(CWordRef{s.cur.data(), 1})) != 2) { fprintf(stderr, "packshim: script: no second election record\n"); return 2; }
    }
    {   // every server holds the entry and votes for itself in term 3: all three voterLog fields are set, and Restart / Timeout of the
        // middle server (evaluated with every other slot of the state) clears its field between two others
        Script s(prm, cv);
        s.leader_with_log(0, 1, true);
        s.restart(0);
        for (int i = 0; i < NS; i++) s.timeout(i);
        for (int i = 0; i < NS; i++) s.request_vote(i, i);
        for (int i = 0; i < NS; i++) if (!s.cur[B::W_VL(i)]) { fprintf(stderr, "packshim: script: voterLog[%d] stayed empty\n", i); return 2; }
    }
    printf("{\"mode\": \"script\", \"words\": [%d, %d], ", B::words(prm), P::words(prm));
    print_cov(cv);
    printf("}\n");
    return 0;
}

static int run_packable() {
    // lb = tb * (MaxClientRequests - 1), tb = 2 while MaxTerm <= 3, else 3
    const int cases[][3] = {{2, 2, 2}, {3, 2, 4}, {4, 3, 2}, {6, 4, 2}, {8, 5, 2}, {9, 4, 4}, {10, 6, 2}};
    printf("{");
    for (size_t k = 0; k < sizeof cases / sizeof cases[0]; k++) {
        const int64_t p[6] = {3, cases[k][1], cases[k][2], 3, 1, 1};
        RaftParams prm;
        if (B::make_params(p, 6, prm) || prm.lb != cases[k][0]) { fprintf(stderr, "packshim: lb of the case is not %d\n", cases[k][0]); return 2; }
        printf("%s\"%d\": %s", k ? ", " : "", prm.lb, P::packable(prm) ? "true" : "false");
    }
    printf("}\n");
    return 0;
}

static int run_field() {
    const int64_t p[10] = {3, 4, 2, 3, 1, 1, 10, 1, 4, 10};   // lb = 6
    RaftParams prm;
    if (B::make_params(p, 10, prm) || prm.lb != 6) return 2;
    const int WB = B::words(prm), WP = P::words(prm);
    std::vector<uint64_t> pub(WB), st(WP), back(WB);
    B::init(prm, 0, WordRef{pub.data(), 1});
    // every bit the base's row can hold next to the entry: an election record with all its bits, the other voterLog entries empty
    pub[B::W_VL(2)] = B::vl_set(0, 2, 0x3f, prm);
    pub[B::W_EL0(prm)] = (1ull << 26) - 1;
    pub[B::W_EL0(prm) + 1] = (1ull << 18) - 1;
    P::import_row(prm, pub.data(), st.data());
    const uint64_t vw = st[P::P_VL];
    const bool placed = vw == (0x3full << (18 * 2 + 6 * 2)), high_clear = (vw >> 54) == 0;
    P::export_row(prm, st.data(), back.data());
    const bool round_trip = back == pub;
    // ... and through the writer: vmode 2 on the Init row, entry (2, 2) all ones
    std::vector<uint64_t> init(WP), out(WP + 1, 0xdeadbeefdeadbeefull);
    P::init(prm, 0, WordRef{init.data(), 1});
    B::Local l;
    P::load(prm, CWordRef{init.data(), 1}, l);
    B::Delta d;
    int action;
    P::compute(prm, l, CWordRef{init.data(), 1}, 0, d, action);   // Restart(s1): a full Delta to start from
    d.srv = 2; d.sv = d.osv = l.sv.get(2); d.log = d.olog = l.log.get(2); d.vmode = 2; d.vj = 2; d.vlog = 0x3f;
    P::store_row(prm, l, CWordRef{init.data(), 1}, d, true, 1, WordRef{out.data(), 1});
    const bool written = out[P::P_VL] == (0x3full << 48) && (out[P::P_VL] >> 54) == 0 && out[WP] == 0xdeadbeefdeadbeefull;
    bool others = true;
    for (int w = 2; w < WP; w++) if (w != P::P_VL && out[w] != init[w]) others = false;
    printf("{\"placed\": %s, \"bit54_and_above_clear\": %s, \"round_trip\": %s, \"writer\": %s, \"other_words_kept\": %s, \"election_word\": %s}\n",
           placed ? "true" : "false", high_clear ? "true" : "false", round_trip ? "true" : "false", written ? "true" : "false", others ? "true" : "false",
           st[P::P_EL0(prm)] == (1ull << 44) - 1 ? "true" : "false");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 8 && !strcmp(argv[1], "bfs")) return run_bfs(argc, argv);
    if (argc >= 11 && !strcmp(argv[1], "walk")) return run_walk(argc, argv);
    if (argc >= 8 && !strcmp(argv[1], "script")) return run_script(argc, argv);
    if (argc == 2 && !strcmp(argv[1], "packable")) return run_packable();
    if (argc == 2 && !strcmp(argv[1], "field")) return run_field();
    fprintf(stderr, "usage: packshim bfs P... | walk SEED N DEPTH P... | script P... | packable | field\n");
    return 2;
}
