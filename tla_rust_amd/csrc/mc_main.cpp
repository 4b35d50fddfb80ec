// mc — command-line front door of libtlamc.so; the drop-in for `tlc X.tla` of the reference's
// Makefile:6-7 / README.md:262 (same inputs: X.tla with X.cfg beside it; same report lines:
// README.md:267-321).  All work happens behind the C ABI (include/tlamc.h).
//
//   mc X.tla [-config X.cfg] [-deadlock] [-workers N] [-device D] [-generic] [-dump FILE] [-dump dot[,actionlabels][,colorize] FILE]
//            [-maxdistinct N] [-maxlevels N] [-tablelog2 T] [-arena N] [-chunk N]
//            [-checkpoint FILE] [-recover FILE] [-gpus P [-samedevice | -torch] [-exchange exact|measured|packed] [-fanout N]] [-noprogress] [-I DIR]
//            [-coverage [MINUTES]] [-strongfair] [-labelfair] [-continue]
//   mc X.tla -simulate [num=N] [-depth D] [-seed S] [-config X.cfg] [-deadlock] [-jit] [-device D] [-noprogress] [-I DIR]
//   mc X.tla -behaviours FILE [-observe v1,v2,...] [-stutter] [-hidden H] [-config X.cfg] [-device D] [-I DIR]
//   mc --transpile X.tla [Y.tla ...]      the `pcal2tla *tla` of the reference's Makefile:3-4: inserts (or
//                                         replaces) the TLA+ translation of the PlusCal algorithm in place,
//                                         the previous text is kept as X.old
//
// A module that has a GPU lowering (the PlusCal programs, raft, the snapshot-isolation and Paxos models) is checked on the GPU
// and nowhere else.  Any OTHER TLA+ module (the Specifying Systems examples of the reference: `mc MCInnerSerial.tla` prints
// testout2:260-266) is evaluated on the host by the general evaluator (csrc/tlaeval.cpp); the report's first line says so.
// -I DIR    : one more directory searched for the modules X.tla EXTENDS / INSTANCEs (after X.tla's own and $TLA_PATH's, which
//             is a ':'-separated list).
// -generic  : check a PlusCal module through the compiled program even when a hand lowering exists.
// -jit      : a compiled PlusCal program runs as GENERATED code — translated to straight-line C++ and built for the device (hipcc) when
//             the engine is created, cached by the program's hash — instead of being interpreted on the device (MC_F_JIT; same report).
//             Without it the search starts on the interpreter and moves to the generated code by itself when it lasts long enough for
//             the build to finish first ($TLAMC_AUTOJIT_AFTER seconds before the build starts, default 0.3; $TLAMC_AUTOJIT=0: never).
// -unverified: an MC wrapper (specs/MCraft.tla ...) EXTENDS a module of the reference (raft.tla); when that module is found
//             neither beside the wrapper nor under $TLA_PATH the run is refused, unless this option accepts the built-in
//             lowering unchecked (the report then starts with a warning).
// -dump FILE: like TLC's -dump, write every distinct state found to FILE.
// -dump dot[,actionlabels][,colorize] FILE: like TLC's, write the state graph to FILE in GraphViz's dot language (mc_engine_graph,
//             mc_check_files_dot): one node per state, one line per transition, with actionlabels the action's name on it, with colorize
//             a colour per action and a legend.  Node k is the state `-dump FILE` prints as "State k:"; both forms may be given in one
//             run and then number the states alike.  The report gains "The state graph has ... states and ... transitions".
// -checkpoint FILE / -recover FILE: TLC's checkpointing (testout1:10) and -recover: write the run (all states found, level
//             boundaries, counters, parent pointers) after a search that stopped on -maxlevels / -maxdistinct without an
//             error; continue such a run later, with the same X.tla / X.cfg.  With -gpus P: one file per rank,
//             FILE.rank<r>of<P> (the rank's arena, parent pointers and seen-set slice); -recover needs the same P.
// -gpus P   : the search sharded over P GPUs of this node, one process per GPU, collectives over RCCL (include/tlamc.h
//             mc_comm_* / mc_shard_run): mc starts P copies of itself (rank r on device r; rank 0 writes the communicator id to
//             a temporary file the others read) and rank 0 prints TLC's counter / depth lines and, on an error, the behaviour that
//             leads to it — walked back across the ranks' arenas (mc_shard_trace); exit status as below.  A rank that fails takes
//             the others down with it (no rank is left waiting in a collective).  -samedevice: every rank on device D (a one-GPU
//             box: only with a librccl stand-in named by $TLAMC_RCCL — RCCL itself refuses two ranks on one device).
// -gpus P -torch: the same search driven by tla_rust_amd/mc_multi.py over torch.distributed instead — mc replaces itself by
//             `python3 -m torch.distributed.run --nproc-per-node P -m tla_rust_amd.mc_multi X.tla <the other options>`; that front
//             door also rebalances drifting ranks by moving states and prints a counterexample walked back across the ranks
//             ($PYTHON names another interpreter, $MASTER_PORT the rendezvous port).
// -simulate [num=N] [-depth D] [-seed S]: TLC's random simulation instead of the exhaustive search — N random walks of at most D
//             states (default 100) from the initial states, every state and successor checked as the search checks them, one GPU
//             lane per walk (mc_engine_simulate).  Without num= it walks until it finds an error or is interrupted (SIGINT: the report
//             of what was walked, exit status 0).  Without -seed a seed is drawn; the report prints it, and the same seed, num and
//             depth give the same walks and the same report.  The report has the error and its behaviour as the search's has, "The
//             number of states generated: G" and the walks, but no distinct-state count or search depth: nothing was searched
//             exhaustively.  -gpus, -dump, -checkpoint and -recover do not apply; a module without a GPU lowering is refused.
// -behaviours FILE [-observe v1,v2,...] [-stutter] [-hidden H]: is every execution recorded in FILE a behaviour of the model (a PlusCal module)?
//             FILE holds states as `mc -dump` / a TLC trace prints them ("State k:" headers are ignored), a blank line between states, a
//             line of ---- between behaviours; a state may leave variables out.  -observe names the variables that count (default: those
//             every state of the file mentions); -stutter lets an observation repeat the state before it; -hidden H (0..255) lets up to H model steps that change no
//             observed variable lie between two observations (the labels an implementation does not log).  One GPU wavefront decides one
//             behaviour (mc_engine_behaviours).  The report counts the verdicts, names the ambiguous behaviours in a warning, and for
//             the first rejected one prints a behaviour of the model up to the observation no step leads to.  Exit status 12 if a
//             behaviour is rejected.  Not with -simulate, -gpus, -recover, -checkpoint, -dump, -coverage or -continue.
// -continue: TLC's -continue: a violated invariant or a deadlock no longer ends the search (MC_F_CONTINUE).  The report prints the first
//             error with its behaviour as ever, then one line per invariant of the model (and one for deadlock): the distinct states
//             that break it — each state under its FIRST violated invariant only —, the violating successors outside the model, the
//             depth of the first one, and its shortest behaviour; a failed Assert or an evaluation error still ends the search and
//             comes last.  The exit status is the first error's.  Not with -simulate, -gpus, -recover or -checkpoint; a module
//             evaluated on the host is refused.
// -coverage [N]: TLC's -coverage: after the search the report lists, for Init and for every action of the model (every label of a PlusCal
//             algorithm and its terminating disjunct), "<Name>: D:G" — the distinct states the action was first to find and the states it
//             generated; an action with 0:0 never fired (MC_F_COVERAGE, mc_engine_coverage).  TLC's argument, the minutes between two
//             reports, is accepted and ignored: the counts are printed once, at the end.  Not with -simulate, -gpus or -recover (a
//             recovered run has no counts for its checkpointed part); a module evaluated on the host gets a warning instead.
// -strongfair: a `fair+ process` of a PlusCal algorithm is checked under strong fairness (MC_F_STRONGFAIR: mc_program_fairness_strong,
//             mc_engine_liveness_strong / mc_engine_liveness_check_strong) instead of being named as NOT checked; an algorithm without
//             `fair+` gets the report it gets without the option.  `+` / `-` labels, procedures, a VIEW and -gpus stay refused.
// -labelfair: liveness under pcal2tla's fairness label by label (MC_F_LABELFAIR: mc_program_fairness_units, mc_engine_liveness_units /
//             mc_engine_liveness_check_units): `fair+`, `l:-` and `l:+` labels and procedures are checked instead of being
//             named as NOT checked; an algorithm with none of them gets the report it gets without the option.  A VIEW and -gpus stay refused.
// -deadlock : as with TLC, do NOT check for deadlock.  -workers is accepted and ignored (the
// GPU is the worker pool).  Exit status: 0 no error, 12 safety violation (invariant / assert),
// 11 deadlock, 1 any other failure — TLC's convention.
#include <errno.h>
#include <limits.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "../../include/tlamc.h"

static int transpile(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "mc: cannot read %s\n", path); return 1; }
    std::string text;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    fclose(f);
    const int need = mc_pcal_translate(text.c_str(), nullptr, 0);
    if (need < 0) { fprintf(stderr, "mc: %s: %s\n", path, mc_last_error()); return 1; }
    std::vector<char> out((size_t)need + 1);
    mc_pcal_translate(text.c_str(), out.data(), out.size());
    std::string old = path;
    const size_t dot = old.rfind(".tla");
    if (dot != std::string::npos) old.replace(dot, 4, ".old"); else old += ".old";
    if ((f = fopen(old.c_str(), "wb"))) { fwrite(text.data(), 1, text.size(), f); fclose(f); }
    if (!(f = fopen(path, "wb"))) { fprintf(stderr, "mc: cannot write %s\n", path); return 1; }
    fwrite(out.data(), 1, (size_t)need, f);
    fclose(f);
    printf("pcal2tla-compatible translation written to %s (previous text in %s)\n", path, old.c_str());
    return 0;
}

// mc X.tla -gpus P ...: hand over to the multi-process front door.  The package root is two directories above this
// binary (tla_rust_amd/_build/mc).
static int exec_multi(int gpus, int argc, char **argv) {
    char exe[PATH_MAX];
    const ssize_t n = readlink("/proc/self/exe", exe, sizeof exe - 1);
    if (n <= 0) { fprintf(stderr, "mc: cannot locate the package root for -gpus\n"); return 1; }
    exe[n] = 0;
    std::string root(exe);
    for (int up = 0; up < 3; up++) { const size_t s = root.rfind('/'); if (s == std::string::npos) break; root.resize(s); }
    const char *pp = getenv("PYTHONPATH");
    setenv("PYTHONPATH", pp && *pp ? (root + ":" + pp).c_str() : root.c_str(), 1);
    const char *port = getenv("MASTER_PORT");
    const char *py = getenv("PYTHON");  // the interpreter that has torch; default: python3 on PATH
    std::vector<std::string> a = {py && *py ? py : "python3", "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=" + std::to_string(gpus),
                                  "--master-addr", "127.0.0.1", "--master-port", port && *port ? port : "29517", "-m", "tla_rust_amd.mc_multi"};
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-gpus")) { ++i; continue; }
        if (!strcmp(argv[i], "-torch") || !strcmp(argv[i], "-samedevice")) continue;
        if (!strcmp(argv[i], "-deadlock") || !strcmp(argv[i], "-dump") || !strcmp(argv[i], "-checkpoint") || !strcmp(argv[i], "-recover")) {
            fprintf(stderr, "mc: %s is not available with -gpus\n", argv[i]);
            return 1;
        }
        a.push_back(argv[i]);
    }
    std::vector<char *> v;
    for (auto &x : a) v.push_back(&x[0]);
    v.push_back(nullptr);
    execvp(v[0], v.data());
    perror("mc: cannot start python3");
    return 1;
}

// ---- mc X.tla -gpus P, native: P copies of this binary, one per GPU, over the hip-rccl back-end of the C ABI
static double now_s() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}
static int spawn_ranks(int gpus, char **argv) {
    char idfile[] = "/tmp/mc_comm_id_XXXXXX";
    const int fd = mkstemp(idfile);
    if (fd < 0) { perror("mc: mkstemp"); return 1; }
    close(fd);  // empty: rank 0 fills it (through a rename), the other ranks wait for MC_COMM_ID_BYTES bytes
    setenv("MC_WORLD", std::to_string(gpus).c_str(), 1);
    setenv("MC_IDFILE", idfile, 1);
    std::vector<pid_t> pids;
    for (int r = 0; r < gpus; r++) {
        const pid_t p = fork();
        if (p < 0) { perror("mc: fork"); return 1; }
        if (p == 0) {
            setenv("MC_RANK", std::to_string(r).c_str(), 1);
            execv("/proc/self/exe", argv);
            perror("mc: exec");
            _exit(1);
        }
        pids.push_back(p);
    }
    int worst = 0;
    size_t left = pids.size();
    while (left) {
        int st = 0;
        const pid_t p = waitpid(-1, &st, 0);
        if (p < 0) break;
        bool ours = false;
        for (pid_t &q : pids) if (q == p) { q = -1; ours = true; }
        if (!ours) continue;
        --left;
        const int code = WIFEXITED(st) ? WEXITSTATUS(st) : 1;
        if (code == 1 || (code > worst && worst != 1)) worst = code;  // 1 (a failure) dominates 11 / 12 (TLC's verdict codes)
        if (code != 0 && code != 11 && code != 12)  // a rank FAILED (a verdict is no failure): the others may be waiting for it in a
            for (pid_t q : pids) if (q > 0) kill(q, SIGTERM);  // collective that will never complete
    }
    unlink(idfile);
    return worst;
}
static uint64_t g_fanout = 0;        // -fanout N: in-model successors per state the buffers of a sharded round allow for (0 = the defaults)
static uint32_t g_shard_flags = 0;  // -exchange exact (default) | measured | packed (mc_shard_opts.flags, include/tlamc.h)
static int run_rank(const char *tla, const char *cfgp, mc_config cfg, int rank, int world, const char *idfile, const char *ckpt, const char *recover) {
    mc_spec_desc desc;
    mc_program *prog = nullptr;
    int rc = mc_resolve_files(tla, cfgp, cfg.flags & (MC_F_GENERIC | MC_F_UNVERIFIED), &desc, &prog);
    if (rc) { fprintf(stderr, "mc[%d]: %s: %s\n", rank, mc_strerror(rc), mc_last_error()); return 1; }
    uint8_t id[MC_COMM_ID_BYTES];
    if (rank == 0) {
        if ((rc = mc_comm_unique_id(id))) { fprintf(stderr, "mc[0]: %s: %s\n", mc_strerror(rc), mc_last_error()); return 1; }
        const std::string tmp = std::string(idfile) + ".w";
        FILE *f = fopen(tmp.c_str(), "wb");
        if (!f || fwrite(id, 1, sizeof id, f) != sizeof id) { perror("mc: communicator id file"); return 1; }
        fclose(f);
        if (rename(tmp.c_str(), idfile)) { perror("mc: rename"); return 1; }
    } else {
        const double t0 = now_s();
        for (;;) {
            FILE *f = fopen(idfile, "rb");
            const size_t n = f ? fread(id, 1, sizeof id, f) : 0;
            if (f) fclose(f);
            if (n == sizeof id) break;
            if (now_s() - t0 > 120) { fprintf(stderr, "mc[%d]: no communicator id from rank 0\n", rank); return 1; }
            usleep(20000);
        }
    }
    if (!getenv("MC_SAMEDEVICE")) cfg.device += rank;  // rank r on device (-device D) + r
    cfg.shard_rank = (uint32_t)rank;
    cfg.shard_count = (uint32_t)world;
    cfg.flags &= ~MC_F_PROGRESS;  // (MC_F_TRACE stays: a counterexample is walked back across the ranks)
    mc_comm *comm = nullptr;
    if ((rc = mc_comm_create(id, (uint32_t)rank, (uint32_t)world, cfg.device, &comm))) { fprintf(stderr, "mc[%d]: %s: %s\n", rank, mc_strerror(rc), mc_last_error()); return 1; }
    mc_engine *eng = nullptr;
    if ((rc = mc_engine_create(&desc, &cfg, &eng))) { fprintf(stderr, "mc[%d]: %s: %s\n", rank, mc_strerror(rc), mc_last_error()); return 1; }
    mc_shard_opts so;
    memset(&so, 0, sizeof so);
    so.flags = g_shard_flags;  // -exchange
    so.packed_fanout = g_fanout;
    so.move_fanout = g_fanout ? 2 * g_fanout : 0;  // (the default pair is 16 / 32)
    so.chunk_states = cfg.chunk_states;
    so.max_distinct = cfg.max_distinct;
    so.max_levels = cfg.max_levels;
    static mc_shard_stats sstats;
    so.stats = &sstats;
    static mc_result res;
    // -recover FILE / -checkpoint FILE with -gpus P: one file per rank, FILE.rank<r>of<P> (mc_shard_restore / mc_shard_checkpoint)
    auto rank_file = [&](const char *stem) { return std::string(stem) + ".rank" + std::to_string(rank) + "of" + std::to_string(world); };
    if (recover && (rc = mc_shard_restore(eng, rank_file(recover).c_str()))) { fprintf(stderr, "mc[%d]: %s: %s\n", rank, mc_strerror(rc), mc_last_error()); return 1; }
    const double t0 = now_s();
    rc = mc_shard_run(eng, comm, &so, &res);
    const double dt = now_s() - t0;
    if (rc) fprintf(stderr, "mc[%d]: %s: %s\n", rank, mc_strerror(rc), mc_last_error());
    if (sstats.restarts && rank == 0)
        fprintf(stderr, "mc: a level had more successors per state than the exchange buckets allow for; the search was started over %llu time(s), "
                        "each with twice the allowance\n", (unsigned long long)sstats.restarts);
    bool ckpt_done = false;
    if (!rc && ckpt && (res.verdict == MC_V_OK || res.verdict == MC_V_BUDGET)) {
        if ((rc = mc_shard_checkpoint(eng, rank_file(ckpt).c_str()))) fprintf(stderr, "mc[%d]: %s: %s\n", rank, mc_strerror(rc), mc_last_error());
        int64_t mine = rc, every[8] = {0};
        const int grc = mc_comm_all_gather(comm, &mine, every, sizeof mine);  // "completed" only when every rank's file is written
        ckpt_done = !grc;
        for (int p = 0; p < world && ckpt_done; p++) ckpt_done = every[p] == 0;
        if (!ckpt_done && !rc) rc = MC_EBADCFG;
    }
    // the behaviour that leads to an error: walked back parent by parent across the ranks (collective: every rank takes part)
    const size_t W = mc_state_bytes(&desc);
    std::vector<uint8_t> tr_states;
    std::vector<int32_t> tr_slots;
    size_t tr_n = 0;
    int32_t tr_final = -1;
    if (!rc && res.verdict != MC_V_OK && res.verdict != MC_V_BUDGET && (cfg.flags & MC_F_TRACE)) {
        tr_n = 4096;
        tr_states.resize(tr_n * W);
        tr_slots.resize(tr_n);
        const int trc = mc_shard_trace(eng, comm, tr_states.data(), tr_slots.data(), &tr_n, &tr_final);
        if (trc) { fprintf(stderr, "mc[%d]: counterexample: %s: %s\n", rank, mc_strerror(trc), mc_last_error()); tr_n = 0; }
    }
    if (!rc && rank == 0) {  // TLC's closing lines (README.md:319-320, testout2:260-266), as tla_rust_amd/mc_multi.py prints them
        const unsigned long long n0 = res.levels ? (unsigned long long)res.level_distinct[0] : 0ull;
        printf("Finished computing initial states: %llu distinct state%s generated.\n", n0, n0 == 1 ? "" : "s");
        // a sharded search keeps no state graph in one place: the cfg's temporal properties are named, never passed over
        // (a PROPERTY that is safety alone — `[]P`, `[][A]_v` — is checked by every rank's `step`, DESIGN section 22: nothing of it is left to name)
        auto safety_alone = [&](const char *name) {
            mc_live_property lp;
            for (int j = 0; mc_program_live_property(prog, j, &lp) == MC_OK; j++)
                if (!strcmp(lp.origin, name)) return lp.refused && !strncmp(lp.reason, "it has no liveness part", 23);
            return false;
        };
        for (int k = 0; prog && mc_program_property(prog, k); k++) {
            if (safety_alone(mc_program_property(prog, k))) continue;
            res.unchecked_properties++;
            printf("Warning: temporal property %s NOT checked: the search is sharded over %d engines (-gpus); liveness needs the state graph of one engine.\n",
                   mc_program_property(prog, k), world);
        }
        if (res.verdict == MC_V_OK) printf("Model checking completed. No error has been found.\n");
        else if (res.verdict == MC_V_BUDGET) printf("Search stopped by the level/state budget; no error has been found so far.\n");
        if (ckpt_done) printf("-- Checkpointing of run %s completed.\n", ckpt);  // testout1:10 (one file per rank: %s.rank<r>of<P>)
        if (res.verdict != MC_V_OK && res.verdict != MC_V_BUDGET) {
            printf("%s\n", res.verdict == MC_V_INVARIANT ? "Error: Invariant is violated." : res.verdict == MC_V_ASSERT ? "Error: The first argument of Assert evaluated to FALSE."
                          : res.verdict == MC_V_DEADLOCK ? "Error: Deadlock reached." : "Error: TLC would raise an evaluation error.");
            if (tr_n) {  // README.md:270-311: "State k: <Action>" + the variables
                printf("Error: The behavior up to this point is:\n");
                std::vector<char> text(1 << 16);
                std::vector<uint8_t> succ(W);
                auto print_state = [&](size_t k, const uint8_t *prev, int32_t slot, const uint8_t *st) {
                    const char *name = "Initial predicate";
                    if (prev) { const int a = mc_state_action(&desc, prev, slot); name = a >= 0 ? mc_action_name(&desc, a) : "?"; }
                    const int n = mc_state_format(&desc, st, text.data(), text.size());
                    printf("State %zu: <%s>\n%.*s\n", k + 1, name, n > 0 ? n : 0, text.data());
                };
                for (size_t k = 0; k < tr_n; k++) print_state(k, k ? &tr_states[(k - 1) * W] : nullptr, tr_slots[k], &tr_states[k * W]);
                if (tr_final >= 0 && mc_state_apply(&desc, &tr_states[(tr_n - 1) * W], tr_final, succ.data()) == 0)
                    print_state(tr_n, &tr_states[(tr_n - 1) * W], tr_final, succ.data());
            } else {
                printf("(no behavior: the engines keep no parent pointers)\n");
            }
        }
        printf("%llu states generated, %llu distinct states found, %llu states left on queue.\n", (unsigned long long)res.generated,
               (unsigned long long)res.distinct, (unsigned long long)res.queue_left);
        printf("The depth of the complete state graph search is %u.\n", res.depth);
        printf("(%d GPU%s over RCCL, %.3f s, %.3g distinct states/s)\n", world, world == 1 ? "" : "s", dt, (double)res.distinct / (dt > 1e-9 ? dt : 1e-9));
        if (world > 1 && sstats.routed_candidates)  // rank 0's share of the exchange: what it handed over against 9 bytes per routed candidate
            printf("(exchange, this rank: %.1f MB of fingerprints and answers for %llu candidates = %.2f x the 9 bytes each needs; %llu stay / %llu move levels)\n",
                   (double)sstats.fp_answer_bytes / 1e6, (unsigned long long)sstats.routed_candidates,
                   (double)sstats.fp_answer_bytes / (9.0 * (double)sstats.routed_candidates), (unsigned long long)sstats.stay_levels,
                   (unsigned long long)sstats.move_levels);
        fflush(stdout);
    }
    mc_engine_destroy(eng);
    mc_comm_destroy(comm);
    if (prog) mc_program_free(prog);
    if (rc) return 1;
    if (res.verdict == MC_V_OK || res.verdict == MC_V_BUDGET) return 0;
    return res.verdict == MC_V_DEADLOCK ? 11 : 12;
}

// a whole decimal number, nothing before or after it (strtoull alone takes "abc" for 0 and "-1" for 2^64 - 1)
static bool parse_u64(const char *s, uint64_t *out) {
    if (!s || *s < '0' || *s > '9') return false;
    errno = 0;
    char *end = nullptr;
    const unsigned long long v = strtoull(s, &end, 10);
    if (errno || *end) return false;
    *out = v;
    return true;
}

// ---- mc X.tla -simulate: the walks of mc_simulate_files; SIGINT stops them between two launches and the report is printed
static volatile sig_atomic_t g_interrupt = 0;
static int run_simulation(const char *tla, const char *cfgp, const mc_config &cfg, mc_sim_opts sim, bool have_seed, const char *refused) {
    if (refused) { fprintf(stderr, "mc: %s is not available with -simulate\n", refused); return 1; }
    if (!have_seed) {   // TLC draws a seed and prints it, so that the run can be repeated
        uint64_t s = (uint64_t)time(nullptr) * 0x9e3779b97f4a7c15ull ^ ((uint64_t)getpid() << 32) ^ (uint64_t)clock();
        FILE *r = fopen("/dev/urandom", "rb");
        if (r) { if (fread(&s, sizeof s, 1, r) != 1) s ^= 0x5851f42d4c957f2dull; fclose(r); }
        sim.seed = s >> 1;   // (non-negative, like TLC's long seeds)
    }
    signal(SIGINT, [](int) { g_interrupt = 1; });
    std::vector<char> report(1 << 22);
    static mc_sim_result res;
    const int rc = mc_simulate_files(tla, cfgp, &cfg, &sim, report.data(), report.size(), &res, (const volatile int *)&g_interrupt);
    signal(SIGINT, SIG_DFL);
    if (rc) {
        fprintf(stderr, "mc: %s: %s\n", mc_strerror(rc), mc_last_error());
        return 1;
    }
    fputs(report.data(), stdout);
    if (res.verdict == MC_V_OK || res.verdict == MC_V_BUDGET) return 0;
    return res.verdict == MC_V_DEADLOCK ? 11 : 12;
}

// ---- mc X.tla -behaviours FILE
static int run_behaviours(const char *tla, const char *cfgp, const mc_config &cfg, const char *file, const char *observe, bool stutter, unsigned hidden) {
    std::vector<char> report(1 << 22);
    mc_beh_result res;
    const int rc = mc_check_behaviours_files(tla, cfgp, &cfg, file, observe, (stutter ? MC_BEH_F_STUTTER : 0u) | MC_BEH_F_HIDDEN(hidden), report.data(), report.size(), &res);
    if (rc) {
        fprintf(stderr, "mc: %s: %s\n", mc_strerror(rc), mc_last_error());
        return 1;
    }
    fputs(report.data(), stdout);
    return res.rejected ? 12 : 0;
}

int main(int argc, char **argv) {
    setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);   // (RCCL between processes needs dmabuf IPC on this driver; read when the HSA runtime starts)
    for (int i = 1; i < argc; i++)   // (before anything else looks at the options)
        if (!strcmp(argv[i], "-behaviours"))
            for (int j = 1; j < argc; j++)
                for (const char *other : {"-simulate", "-gpus", "-recover", "-checkpoint", "-dump", "-coverage", "-continue"})
                    if (!strcmp(argv[j], other)) { fprintf(stderr, "mc: %s is not available with -behaviours\n", other); return 1; }
    int gpus = 0;
    bool torch_door = false;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-gpus") && i + 1 < argc) {
            gpus = atoi(argv[i + 1]);
            if (gpus < 1 || gpus > 64) { fprintf(stderr, "mc: -gpus needs a number of GPUs\n"); return 1; }
        }
        if (!strcmp(argv[i], "-torch")) torch_door = true;
        if (!strcmp(argv[i], "-samedevice")) setenv("MC_SAMEDEVICE", "1", 1);
    }
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "-simulate") && gpus) { fprintf(stderr, "mc: -gpus is not available with -simulate\n"); return 1; }
    for (int i = 1; i < argc; i++)   // (before any rank is started, and before anything touches a device)
        if (!strcmp(argv[i], "-coverage"))
            for (int j = 1; j < argc; j++)
                for (const char *other : {"-simulate", "-gpus", "-recover"})
                    if (!strcmp(argv[j], other)) { fprintf(stderr, "mc: -coverage is not available with %s\n", other); return 1; }
    for (int i = 1; i < argc; i++)
        if (!strcmp(argv[i], "-continue"))
            for (int j = 1; j < argc; j++)
                for (const char *other : {"-simulate", "-gpus", "-recover", "-checkpoint"})
                    if (!strcmp(argv[j], other)) { fprintf(stderr, "mc: -continue is not available with %s\n", other); return 1; }
    if (gpus && !getenv("MC_RANK"))
        for (int i = 1; i < argc; i++)
            if (!strcmp(argv[i], "-dump") && i + 1 < argc && (!strcmp(argv[i + 1], "dot") || !strncmp(argv[i + 1], "dot,", 4))) {
                fprintf(stderr, "mc: -dump is not available with -gpus\n");
                return 1;
            }
    if (gpus && torch_door) return exec_multi(gpus, argc, argv);
    const char *env_rank = getenv("MC_RANK");
    if (gpus && !env_rank) {
        if (gpus > 8) { fprintf(stderr, "mc: -gpus: at most 8 ranks (one node)\n"); return 1; }
        return spawn_ranks(gpus, argv);
    }
    if (argc >= 2 && (!strcmp(argv[1], "--transpile") || !strcmp(argv[1], "-transpile"))) {
        int rc = argc > 2 ? 0 : 1;
        for (int i = 2; i < argc; i++) rc |= transpile(argv[i]);
        return rc;
    }
    const char *tla = nullptr, *cfgp = nullptr, *dump = nullptr, *recover = nullptr, *ckpt = nullptr, *dot = nullptr;
    unsigned dot_flags = 0;
    bool simulate = false, have_seed = false, have_depth = false, stutter = false;
    const char *beh_file = nullptr, *observe = nullptr;
    uint64_t hidden = 0;
    bool have_hidden = false;
    mc_sim_opts sim;
    memset(&sim, 0, sizeof sim);
    sim.depth = 100;   // TLC's default -depth
    mc_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.flags = MC_F_DEADLOCK | MC_F_TRACE | MC_F_PROGRESS;  // TLC reports its progress while it runs (testout2:4-259); -noprogress
    cfg.table_capacity = 1ull << 26;
    cfg.arena_capacity = 1ull << 24;
    for (int i = 1; i < argc; i++) {
        auto arg = [&](const char *name) { return !strcmp(argv[i], name) && i + 1 < argc; };
        if (arg("-config")) cfgp = argv[++i];
        else if (!strcmp(argv[i], "-simulate")) {
            simulate = true;
            if (i + 1 < argc && !strncmp(argv[i + 1], "num=", 4)) {
                if (!parse_u64(argv[++i] + 4, &sim.num) || !sim.num || sim.num > (1ull << 40)) {
                    fprintf(stderr, "mc: -simulate num=N needs a number of walks (1..2^40)\n");
                    return 1;
                }
            }
        }
        else if (arg("-depth")) {
            uint64_t v = 0;
            if (!parse_u64(argv[++i], &v) || v < 1 || v > MC_SIM_MAX_DEPTH) { fprintf(stderr, "mc: -depth needs a number of states (1..%d)\n", MC_SIM_MAX_DEPTH); return 1; }
            sim.depth = (uint32_t)v;
            have_depth = true;
        }
        else if (arg("-seed")) {
            if (!parse_u64(argv[++i], &sim.seed)) { fprintf(stderr, "mc: -seed needs a non-negative integer\n"); return 1; }
            have_seed = true;
        }
        else if (!strcmp(argv[i], "-coverage")) {
            cfg.flags |= MC_F_COVERAGE;
            uint64_t minutes = 0;   // TLC's interval between two coverage reports: accepted, not used
            if (i + 1 < argc && parse_u64(argv[i + 1], &minutes)) ++i;
        }
        else if (!strcmp(argv[i], "-continue")) cfg.flags |= MC_F_CONTINUE;
        else if (arg("-behaviours")) beh_file = argv[++i];
        else if (arg("-observe")) observe = argv[++i];
        else if (!strcmp(argv[i], "-stutter")) stutter = true;
        else if (arg("-hidden")) {
            if (!parse_u64(argv[++i], &hidden) || hidden > MC_BEH_MAX_HIDDEN) {
                fprintf(stderr, "mc: -hidden needs a number of unlogged steps between observations (0..%d)\n", MC_BEH_MAX_HIDDEN);
                return 1;
            }
            have_hidden = true;
        }
        else if (!strcmp(argv[i], "-deadlock")) cfg.flags &= ~MC_F_DEADLOCK;
        else if (arg("-dump") && (!strcmp(argv[i + 1], "dot") || !strncmp(argv[i + 1], "dot,", 4))) {   // TLC: -dump dot[,actionlabels][,colorize] FILE
            for (const char *s = argv[++i] + 3; *s;) {
                const char *e = strchr(++s, ',');
                const std::string sub(s, e ? (size_t)(e - s) : strlen(s));
                if (sub == "actionlabels") dot_flags |= MC_DOT_ACTIONLABELS;
                else if (sub == "colorize") dot_flags |= MC_DOT_COLORIZE;
                else { fprintf(stderr, "mc: unknown -dump option %s\n", sub.c_str()); return 1; }
                s += sub.size();
            }
            if (i + 1 >= argc) { fprintf(stderr, "mc: -dump dot needs a file name\n"); return 1; }
            dot = argv[++i];
        }
        else if (arg("-dump")) dump = argv[++i];
        else if (arg("-checkpoint")) ckpt = argv[++i];
        else if (arg("-recover")) recover = argv[++i];
        else if (arg("-workers")) ++i;
        else if (arg("-gpus")) ++i;
        else if (arg("-fanout")) {  // a dense model (the SI specs: up to ~40 in-model successors per state) without the restarts that find the allowance by doubling
            g_fanout = strtoull(argv[++i], nullptr, 10);
            if (g_fanout < 1 || g_fanout > 4096) { fprintf(stderr, "mc: -fanout needs a number of successors per state (1..4096)\n"); return 1; }
        }
        else if (arg("-exchange")) {  // how the stay levels of a -gpus run exchange their candidates (MC_SHARD_*)
            const char *v = argv[++i];
            if (!strcmp(v, "packed")) g_shard_flags = MC_SHARD_PACKED | MC_SHARD_FIXED_CAPS;
            else if (!strcmp(v, "measured")) g_shard_flags = MC_SHARD_PACKED;
            else if (!strcmp(v, "exact")) g_shard_flags = 0;
            else { fprintf(stderr, "mc: -exchange exact | measured | packed\n"); return 1; }
        }
        else if (!strcmp(argv[i], "-torch") || !strcmp(argv[i], "-samedevice")) {}
        else if (!strcmp(argv[i], "-generic")) cfg.flags |= MC_F_GENERIC;
        else if (!strcmp(argv[i], "-jit")) cfg.flags |= MC_F_JIT;
        else if (!strcmp(argv[i], "-unverified")) cfg.flags |= MC_F_UNVERIFIED;
        else if (!strcmp(argv[i], "-strongfair")) cfg.flags |= MC_F_STRONGFAIR;
        else if (!strcmp(argv[i], "-labelfair")) cfg.flags |= MC_F_LABELFAIR;
        else if (arg("-I")) {  // one more directory searched for EXTENDed / INSTANCEd modules (appended to $TLA_PATH)
            const char *old = getenv("TLA_PATH");
            const std::string v = old && *old ? std::string(old) + ":" + argv[i + 1] : std::string(argv[i + 1]);
            setenv("TLA_PATH", v.c_str(), 1);
            ++i;
        }
        else if (!strcmp(argv[i], "-noprogress")) cfg.flags &= ~MC_F_PROGRESS;
        else if (arg("-device")) cfg.device = atoi(argv[++i]);
        else if (arg("-maxdistinct")) cfg.max_distinct = strtoull(argv[++i], 0, 10);
        else if (arg("-maxlevels")) cfg.max_levels = strtoull(argv[++i], 0, 10);
        else if (arg("-tablelog2")) cfg.table_capacity = 1ull << atoi(argv[++i]);
        else if (arg("-table")) cfg.table_capacity = strtoull(argv[++i], 0, 10);  // seen-set slots, any number
        else if (arg("-arena")) cfg.arena_capacity = strtoull(argv[++i], 0, 10);
        else if (arg("-chunk")) cfg.chunk_states = strtoull(argv[++i], 0, 10);
        else if (!strcmp(argv[i], "-help") || !strcmp(argv[i], "--help") || !strcmp(argv[i], "-h")) { tla = nullptr; break; }
        else if (argv[i][0] != '-') tla = argv[i];
        else { fprintf(stderr, "mc: unknown option %s\n", argv[i]); return 1; }
    }
    if (!tla) {
        fprintf(stderr,
                "usage: mc X.tla [-config X.cfg] [-deadlock] [-dump FILE] [-generic] [-jit] [-unverified] [-device D] [-I DIR]\n"
                "                [-dump dot[,actionlabels][,colorize] FILE]                               ... and write the state graph (node k = State k of -dump FILE)\n"
                "                [-maxdistinct N] [-maxlevels N] [-tablelog2 T] [-arena N] [-chunk N]\n"
                "                [-checkpoint FILE] [-recover FILE] [-gpus P [-torch]]                    check X.tla like `tlc X.tla`\n"
                "                [-coverage [MINUTES]]                                                    ... and list every action's distinct:generated counts\n"
                "                [-continue]                                                              ... and search on past violated invariants and deadlocks:\n"
                "                the first error as ever, then every invariant with its number of violating states and a shortest behaviour\n"
                "                a PlusCal X.tla whose X.cfg says PROPERTY Termination: checked under the algorithm's weak fairness (`fair process`,\n"
                "                `--fair algorithm`) on the complete state graph; so is a PROPERTY that names a definition of the shape <>A, []<>A,\n"
                "                <>[]A or A ~> B over state predicates (under \\A over constant sets, and conjunctions of these); any other temporal\n"
                "                property is named as NOT checked, with the reason\n"
                "                [-strongfair]                                                            ... and check a `fair+ process` under strong fairness\n"
                "                (SF: a process enabled again and again must step) instead of naming its properties as NOT checked; `+` / `-` labels stay refused\n"
                "                [-labelfair]                                                             ... and check under pcal2tla's fairness label by label:\n"
                "                `fair+`, a label `l:-` (left out of its conjunct), a label `l:+` (SF of that action alone), a conjunct per procedure a fair process calls\n"
                "                a PlusCal X.tla whose X.cfg says ACTION_CONSTRAINT A: a step that violates A is generated and its successor checked,\n"
                "                but not stored; VIEW V (a tuple of variables and scalar expressions): a state is fingerprinted by its view, the\n"
                "                first state to arrive stands for its view value.  As with TLC: unless equal views imply equal futures, WHICH state\n"
                "                that is depends on the order of arrival within a level, and the counts may differ from run to run; a temporal\n"
                "                property under a VIEW is named as NOT checked\n"
                "       mc X.tla -simulate [num=N] [-depth D] [-seed S] [...]                             random walks like `tlc -simulate`\n"
                "       mc X.tla -behaviours FILE [-observe v1,v2,...] [-stutter] [-hidden H]             is every execution recorded in FILE a behaviour of the model?\n"
                "       mc --transpile X.tla [Y.tla ...]                                                  translate like `pcal2tla`\n"
                "exit status: 0 no error, 12 invariant / assertion violated, 11 deadlock, 13 a temporal property violated, 1 anything else\n");
        return 1;
    }
    if (!simulate && (have_depth || have_seed)) { fprintf(stderr, "mc: %s needs -simulate\n", have_depth ? "-depth" : "-seed"); return 1; }
    if (!beh_file && (observe || stutter || have_hidden)) {
        fprintf(stderr, "mc: %s needs -behaviours\n", observe ? "-observe" : stutter ? "-stutter" : "-hidden");
        return 1;
    }
    if (beh_file) {
        cfg.flags &= ~(unsigned)MC_F_PROGRESS;
        cfg.table_capacity = 1ull << 16;   // (no search runs: the seen-set and the arena stay empty)
        cfg.arena_capacity = 1ull << 14;
        return run_behaviours(tla, cfgp, cfg, beh_file, observe, stutter, (unsigned)hidden);
    }
    if (simulate) return run_simulation(tla, cfgp, cfg, sim, have_seed, dump || dot ? "-dump" : ckpt ? "-checkpoint" : recover ? "-recover" : nullptr);
    if (gpus) {  // one rank of `mc X.tla -gpus P`
        if (dump || dot) { fprintf(stderr, "mc: -dump is not available with -gpus\n"); return 1; }
        return run_rank(tla, cfgp, cfg, atoi(env_rank), gpus, getenv("MC_IDFILE"), ckpt, recover);
    }
    std::vector<char> report(1 << 22);
    static mc_result res;
    const int rc = dot ? mc_check_files_dumps(tla, cfgp, &cfg, report.data(), report.size(), &res, dump, dot, dot_flags, recover, ckpt)
                       : mc_check_files_ckpt(tla, cfgp, &cfg, report.data(), report.size(), &res, dump, recover, ckpt);
    if (rc) {
        fprintf(stderr, "mc: %s: %s\n", mc_strerror(rc), mc_last_error());
        return 1;
    }
    fputs(report.data(), stdout);
    if (res.verdict == MC_V_OK || res.verdict == MC_V_BUDGET) return 0;
    if (res.verdict == MC_V_LIVENESS) return 13;   // TLC's exit status for a violated liveness property
    return res.verdict == MC_V_DEADLOCK ? 11 : 12;
}
