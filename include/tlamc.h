/*
 * include/tlamc.h — C ABI of libtlamc.so, the MI355X-native explicit-state model checker
 * for the spacejam/tla-rust specs.
 *
 * The reference has no FFI of its own: its boundary is the command line `tlc X.tla` with
 * `X.cfg` beside it (reference Makefile:6-7, README.md:262,356) and TLC's stdout report
 * (README.md:267-321).  BASELINE.json:north_star asks for a host (Rust in intent) that calls
 * HIP "through a thin C-ABI FFI"; this header IS that FFI.  Every entry point below names the
 * part of the reference's workflow it replaces.  Plain pointers and sizes only; the caller
 * owns every *out buffer, the engine owns all device memory; no function throws or aborts
 * across the boundary: each returns 0 or a negative MC_E* code (mc_strerror()).
 *
 * There is no CPU fallback behind this ABI: every function that computes needs a HIP device
 * (gfx950) and fails with MC_EHIP without one.
 */
#ifndef TLAMC_H
#define TLAMC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ error codes */
#define MC_OK 0
#define MC_EBADCFG (-1)    /* bad spec id / constants / configuration                        */
#define MC_EHIP (-2)       /* HIP runtime error or no device                                 */
#define MC_EOVERFLOW (-3)  /* a fixed-capacity slot array of the packed state overflowed     */
#define MC_ETABLEFULL (-4) /* seen-set load factor exceeded                                  */
#define MC_EARENA (-5)     /* state arena (frontier storage) exhausted                       */
#define MC_ERCCL (-6)      /* exchange failure in sharded mode                               */
#define MC_ESTATE (-7)     /* call sequence error                                            */
#define MC_EPARSE (-8)     /* .cfg / .tla front-end error                                    */
#define MC_ENOSPEC (-9)    /* module is not one of the lowered specs (or its text changed)   */
#define MC_EROUTE (-10)    /* sharded mode: an exchange bucket of a round was too small for the candidates it had to hold
                            * (mc_shard_opts.packed_fanout / move_fanout); nothing was truncated.  mc_shard_run* does not hand
                            * this to its caller until it has restarted the search with twice the allowance (mc_shard_stats.restarts) */

/* ------------------------------------------------------------------ verdicts (TLC's outcomes) */
#define MC_V_OK 0          /* "Model checking completed. No error has been found." (testout2:260) */
#define MC_V_INVARIANT 1   /* an INVARIANT of the cfg is violated (pcal_intro.cfg:3)          */
#define MC_V_ASSERT 2      /* "The first argument of Assert evaluated to FALSE" (README.md:268) */
#define MC_V_DEADLOCK 3    /* p-manual §4.7.1 p.41                                            */
#define MC_V_SPECERR 4     /* TLC would raise an evaluation error (index out of domain)       */
#define MC_V_BUDGET 5      /* stopped by max_levels / max_distinct                            */
#define MC_V_ASSUME 6      /* an ASSUME of the module is false (TLC's "No Behavior Spec" mode: a cfg that names neither SPECIFICATION
                            * nor INIT / NEXT — SpecifyingSystems/SimpleMath/SimpleMath.cfg — makes mc_check_files evaluate the ASSUMEs) */
#define MC_V_LIVENESS 7    /* "Temporal properties were violated": PROPERTY Termination of a fair PlusCal algorithm (mc_check_files only:
                            * the search's own verdict was MC_V_OK; mc_engine_liveness decided on its state graph)                      */

/* ------------------------------------------------------------------ lowered specs */
#define MC_SPEC_ATOMIC_ADD 1 /* reference atomic_add.tla:4-23, N adders + checker; params {N}          */
#define MC_SPEC_PCAL_INTRO 2 /* reference pcal_intro.tla:4-23; params {variant, checkInv, MaxMoney, P}  */
#define MC_SPEC_RAFT 3       /* reference examples/raft.tla:110-507 under specs/MCraft.tla;
                                params {nServer, MaxClientRequests, MaxTerm, MaxLogLen, MaxMsgs,
                                        invariantMask (1 NoTwoLeaders | 2 CommittedLogStable),
                                        [6..8] capacities of the messages / elections / allLogs slot arrays of the
                                        packed state (0 = default 40 / 4 / 16; exceeding one is MC_EOVERFLOW),
                                        [9] MaxMsgKeys (0 = unbounded)}                             */

#define MC_SPEC_SSI 4        /* reference examples/serializableSnapshotIsolation.tla:219-996 under specs/MCssi.tla;
                                params {nTxn <= 4, nKey <= 3, invariantMask (1 WellFormed | 2 HoldingXLocks |
                                4 WaitingForXLock | 8 CorrectReadView | 16 FirstCommitterWins | 32 Cahill |
                                64 Bernstein), find (0; 1..6 abort reason, 7 two waiters: ":81-96 expected"),
                                textbook (1 = examples/textbookSnapshotIsolation.tla: no Cahill variables)}  */

#define MC_SPEC_PCAL 5       /* a PlusCal algorithm compiled by mc_program_compile (any module of the supported subset,
                                the reference's untranslated pcal_intro.tla:4-19 and atomic_add.tla:4-23 included);
                                params {(int64) mc_program handle} — build the descriptor with mc_program_spec      */

#define MC_SPEC_PAXOS 6      /* reference examples/Paxos/Voting.tla:133-160 and Paxos.tla:93-208 under MCVoting.tla / MCPaxos.tla
                                (+ .cfg: INVARIANT, PROPERTY C!Spec / V!Spec as a per-transition refinement check, SYMMETRY);
                                params {kind (0 Paxos, 1 Voting), nAcceptor <= 4, nValue <= 3, nBallot = MaxBallot + 1 <= 4,
                                invariantMask (Paxos: bit k = Inv!(k+1), MCPaxos.tla:65-68; Voting: 1 = Inv),
                                symmetry (1 Permutations(Acceptor) | 2 Permutations(Value)),
                                property (1 = check the cfg's PROPERTY; a violation is reported as invariant index 4 (Paxos) /
                                1 (Voting); 2 = negative control: Phase2a without its quorum conjunct),
                                nQuorum (0 = all majorities of minimal size), quorum acceptor bit masks ...}            */

typedef struct {
    uint32_t spec_id;
    uint32_t nparams;
    int64_t params[16];
} mc_spec_desc;

#define MC_F_DEADLOCK 1u /* check deadlock (TLC default on; serializableSnapshotIsolation.tla:57) */
#define MC_F_TRACE 2u    /* keep (parent, action) per state so a counterexample can be rebuilt     */
#define MC_F_TIMING 4u   /* time every kernel launch with HIP events on the engine stream          */
#define MC_F_MATRIX 8u   /* A/B only: unfused expand -> candidate matrix -> insert kernels          */
#define MC_F_NOPROBE 16u /* profiling only (mc_engine_debug_reexpand): skip the seen-set probes   */
#define MC_F_NOFAMILY 32u /* A/B only: expand raft slot by slot instead of by action family        */
#define MC_F_OCC3 2048u      /* A/B only: the by-family expand kernel compiled for 3 wavefronts per SIMD (146 VGPRs, no spills) instead of 4 */
#define MC_F_NOINWAVE 65536u /* A/B only: every new state through the new-list and k_materialise (rounds 1-3) instead of being written by
                                the expand wavefront that found it (round 4; by-family kernels of a fused run) */
#define MC_F_WAVETAIL 131072u /* A/B only: in-wave writes by wavefront (no workgroup barrier) instead of by workgroup */
#define MC_F_PARK 32768u /* measured, not the default (round 6): a by-family wavefront whose survivor list fills up PARKS the overflow in the
                           * new-list's memory and the workgroup's own tail writes it in later rounds (k_expand_family<.., PARK>), instead of
                           * sending it through the new-list to k_materialise: every state is written in-wave, the step takes as long */
#define MC_F_NOFILTER 8192u  /* A/B only: by-family expand kernel without the per-wavefront duplicate filter in front of the seen-set */
#define MC_F_SYNCPROBE 4096u /* A/B only: the by-family expand kernel waits for every seen-set probe where it issues it (rounds 1-4) instead of
                              * resolving a batch of probes one batch later (round 5: split-phase probes, engine.hip MC_ASYNC_PROBE) */
#define MC_F_PROGRESS 16384u /* mc_check_files: print TLC's "Progress(d): ..." lines (testout2:4-259) to stdout while the search runs,
                              * at most one per second */
#define MC_F_NOBATCH 256u /* A/B only: one host round trip per BFS level even while the frontier is small         */
#define MC_F_UNVERIFIED 512u /* mc_check_files / mc_resolve_files: when the module an MC wrapper EXTENDS (raft.tla, the snapshot-isolation
                             specs) is found neither beside it nor under $TLA_PATH, use the built-in lowering anyway (the report
                             carries a warning) instead of failing with MC_ENOSPEC                                          */
#define MC_F_JIT 262144u /* MC_SPEC_PCAL engines: translate the compiled program into straight-line C++ (mc_program_codegen) and build it for
                            the device when the engine is created (hipcc, cached by the hash of the text: seconds to a minute the first
                            time) instead of interpreting its bytecode on the device; $TLAMC_JIT=1 does the same for every such engine.
                            Same states and counts; the engine STORES its rows packed to the cells' inferred ranges (an interval analysis
                            of the program; $TLAMC_JIT_PACK=0: 32 bits per cell like the interpreter) and hands them out — mc_engine_trace,
                            mc_engine_read_states — as the interpreter's rows, mc_state_bytes(spec) each; a checkpoint of packed rows is
                            continued by an engine of the same generated code only (mc_check_files' recover path tries that by itself);
                            the mc_shard_* entry points refuse a packed engine (a config with shard_count > 1 is built unpacked).
                            A program the translator does not cover (sets of records) or a box without hipcc falls back to the
                            interpreter and says so on stderr */
#define MC_F_GENERIC 128u /* mc_check_files: run a PlusCal module through the compiled program (MC_SPEC_PCAL) even
                             when a hand lowering of its algorithm exists (A/B of the two paths)  */
#define MC_F_STRONGFAIR 33554432u /* mc_check_files (`mc -strongfair`): a `fair+ process` is checked under strong fairness (mc_program_fairness_strong,
                             mc_engine_liveness_strong / mc_engine_liveness_check_strong) instead of being named as NOT checked.  Without
                             `fair+` in the algorithm the report is the one without the flag. */
#define MC_F_LABELFAIR 134217728u /* mc_check_files (`mc -labelfair`): liveness under pcal2tla's fairness label by label — `fair+`, `+` / `-` labels,
                             procedures — by units and conjuncts (mc_program_fairness_units, mc_engine_liveness_units /
                             mc_engine_liveness_check_units) instead of naming the properties as NOT checked.  Without it every report is
                             what it was; a program with none of these forms gets the same report with it. */
#define MC_F_COVERAGE 16777216u /* TLC's -coverage: count, per action of the model, the successors it generated and the distinct states it
                             was first to find (mc_engine_coverage below; mc_check_files appends "The coverage statistics" to its
                             report).  Implies MC_F_TRACE.  One-GPU engines only: mc_engine_create refuses it with shard_count > 1.
                             (Bits 19 - 23 are the kernels' own: engine_kernels.h.)  Without it nothing is launched or allocated for it. */
#define MC_F_CONTINUE 67108864u /* TLC's -continue: a violated INVARIANT and a deadlock (MC_F_DEADLOCK) no longer end the search; a failed
                             Assert, an evaluation error and every device error still end it at the end of their level.  mc_result's
                             verdict, violated_invariant and trace_len, and mc_engine_trace, stay those of the FIRST flagged level;
                             mc_engine_violations below lists everything found.  Implies MC_F_TRACE.  One-GPU engines only:
                             mc_engine_create refuses it with shard_count > 1.  Without it nothing is launched or allocated for it. */

typedef struct {
    int32_t device;          /* HIP device ordinal                                              */
    uint32_t flags;          /* MC_F_*                                                          */
    uint64_t table_capacity; /* seen-set slots, ANY number (rounded up to whole 64-slot groups; 0 = default 2^24):
                                size it to the HBM that is left, not to a power of two             */
    uint64_t arena_capacity; /* states kept resident in HBM (0 = default)                       */
    uint64_t chunk_states;   /* frontier states expanded per launch (0 = default)               */
    uint64_t max_levels;     /* 0 = unlimited                                                   */
    uint64_t max_distinct;   /* 0 = unlimited; stop after the level whose cumulative D >= it    */
    uint32_t shard_rank;     /* fingerprint-sharded mode: this engine's rank ...                */
    uint32_t shard_count;    /* ... of shard_count (0 or 1 = single GPU)                        */
} mc_config;

#define MC_MAX_LEVELS 4096

typedef struct {
    uint64_t distinct;        /* "distinct states found"   (README.md:319)                      */
    uint64_t generated;       /* "states generated"        (README.md:319)                      */
    uint64_t queue_left;      /* "states left on queue"    (README.md:319)                      */
    uint32_t depth;           /* "The depth of the complete state graph search is D." (README.md:320) */
    int32_t verdict;          /* MC_V_*                                                         */
    int32_t violated_invariant; /* index into the spec's invariant list, -1 if none             */
    uint32_t trace_len;       /* states in the counterexample, 0 if none                        */
    uint32_t levels;          /* entries valid in level_distinct[]                              */
    uint32_t host_evaluated;  /* 1: mc_check_files ran a module WITHOUT a GPU lowering on the host's general TLA+ evaluator */
    uint32_t unchecked_properties; /* cfg PROPERTIES with a liveness part (<>, ~>, WF_ / SF_) that were NOT checked: only their safety
                                 parts ([]P, [][A]_v, initial predicates) are; the report names them in a "Warning:" line.  A caller
                                 that needs TLC's verdict on them must not read "No error has been found" as that verdict. */
    double seconds;           /* init -> last level complete, device work included              */
    uint64_t level_distinct[MC_MAX_LEVELS]; /* new distinct states per BFS level                */
} mc_result;

/* per-kernel timing, measured with HIP events on the engine's own stream */
typedef struct {
    uint64_t launches;
    double ms_total;
    uint64_t units;           /* states (expand/materialise) or candidates (insert) processed   */
} mc_kernel_stat;
typedef struct {
    mc_kernel_stat expand, insert, materialise;
    uint64_t state_bytes;     /* W: packed bytes per state in HBM                               */
    uint64_t cand_cells;      /* candidate-matrix cells probed                                  */
    uint64_t inwave_states;   /* states the expand wavefronts wrote themselves (the others went through k_materialise) */
} mc_kernel_stats;

typedef struct mc_engine mc_engine;

/* ------------------------------------------------------------------ whole-run API
 * Together these replace the BFS inside `tlc X.tla` (reference Makefile:6-7): initial-state
 * enumeration, successor generation, fingerprinting, seen-set, invariant / Assert / deadlock
 * checks, counters, depth and counterexample (README.md:267-321, testout2:1-266). */
int mc_engine_create(const mc_spec_desc *spec, const mc_config *cfg, mc_engine **out);
int mc_engine_run(mc_engine *e, mc_result *out);
/* Incremental search: `levels` more BFS levels.  The first call starts from Init (like mc_engine_run with max_levels = levels);
 * a call after a step that stopped at its budget (MC_V_BUDGET) continues where it stopped — arena, seen-set and parent pointers
 * stay resident in HBM, nothing is recomputed; `out` holds the counters of the whole search so far.  After a step that ended
 * the search (MC_V_OK) or found an error, the next call starts over.  cfg.max_distinct still applies. */
int mc_engine_step(mc_engine *e, uint32_t levels, mc_result *out);
/* Progress reports while mc_engine_run searches (TLC's "Progress(5): 6117 states generated, 195 distinct states found, 1 states
 * left on queue.", testout2:4-259): `fn` is called from the calling thread between two BFS levels, at most once per
 * `min_interval_seconds`, with the number of levels found so far and the three counters.  fn = NULL switches it off. */
typedef void (*mc_progress_fn)(void *user, uint32_t levels, uint64_t generated, uint64_t distinct, uint64_t queue);
int mc_engine_set_progress(mc_engine *e, mc_progress_fn fn, void *user, double min_interval_seconds);
/* From inside a progress callback: the running mc_engine_run / mc_engine_step stops before its next BFS level as if its budget
 * were spent (MC_V_BUDGET; everything searched so far stays resident, mc_engine_step continues it).  TLC has no counterpart (one
 * interrupts it with ^C and -recover's from the last checkpoint); `mc` uses it to move a compiled PlusCal program from the device
 * interpreter to generated code once that is built. */
int mc_engine_request_stop(mc_engine *e);
/* counterexample of the last run: states_out receives trace_len records of mc_state_bytes()
 * bytes each (plain word order), actions_out the action id that produced each state (-1 for
 * the initial state).  *n_inout: capacity in, count out. */
int mc_engine_trace(mc_engine *e, uint8_t *states_out, int32_t *actions_out, size_t *n_inout);
int mc_engine_kernel_stats(mc_engine *e, mc_kernel_stats *out);

/* ------------------------------------------------------------------ coverage (TLC's `-coverage`)
 * "Did every action of my spec ever fire?"  An engine created with MC_F_COVERAGE counts, while it searches (breadth-first search
 * only: mc_engine_run / mc_engine_step), per action id of the model (mc_action_name) and for Init (action id -1):
 *   generated[a]  the successors counted in mc_result.generated that action a produced: every (expanded state, slot) pair whose
 *                 evaluation is enabled — a failed Assert, an evaluation error, an out-of-model successor and a self loop count too,
 *                 exactly as they count in mc_result.generated.  generated[Init] = the initial states generated.  The sum over the
 *                 entries is mc_result.generated.
 *   distinct[a]   the stored states whose recorded (parent, slot) is action a, i.e. the states a was FIRST to find;
 *                 distinct[Init] = the stored initial states.  The sum is mc_result.distinct.  When two actions reach the same new
 *                 state within one level, which of them is credited is the engine's race (as it is TLC's with several workers):
 *                 generated[] is a function of the model, distinct[] only between bounds (DESIGN.md "Coverage").
 * The levels covered are exactly the levels the search expanded: counting stops where the search stops (max_levels / max_distinct,
 * or the end of the level that found a violation).  mc_engine_step accumulates across the calls that continue one search; a search
 * that starts over starts its counts over.  A run that continues a restored checkpoint recounts the checkpointed levels from the
 * arena and the parent pointers the file brought.  An action with 0 : 0 never fired: a guard that cannot hold, a label no process reaches.
 * Compiled PlusCal programs (interpreted or MC_F_JIT) have one entry per label and one for the terminating disjunct ("Terminating").
 * mc_engine_coverage: the entries for Init and every action of the model, in action-id order, zero rows included.  *n_inout: capacity
 * in, count out (MC_EBADCFG with the count when the buffer is too small).  MC_ESTATE on an engine created without MC_F_COVERAGE. */
typedef struct {
    int32_t action;           /* action id (mc_action_name), -1 = Init                                   */
    uint32_t pad;
    uint64_t distinct, generated;
} mc_action_coverage;
int mc_engine_coverage(mc_engine *e, mc_action_coverage *out, size_t *n_inout);

/* ------------------------------------------------------------------ every violation of a search (TLC's `-continue`)
 * An engine created with MC_F_CONTINUE searches on past violated invariants and deadlocks and collects, per flagged BFS level (two
 * passes over that level alone; a level without a violation costs nothing):
 *   one entry per INVARIANT index of the model, in index order, zero rows included (mc_invariant_name names them);
 *   then one entry for deadlock when MC_F_DEADLOCK is set;
 *   then one entry for the fatal error — a failed Assert, an evaluation error — if one ended the run.
 * states       distinct STORED states: those whose FIRST violated invariant is this one (a state is listed under one invariant only, as
 *              TLC lists it), or the deadlocked states; each state once, however many parents generated it.
 * outside      violating successors that are not stored (outside the CONSTRAINT, refused by an ACTION_CONSTRAINT), counted per
 *              generation; always 0 for a lowering that checks stored states.  The fatal entry: the failing (state, action) pairs
 *              of the level that ended the run.
 * first_state  arena index of the first violator (the arena is in level order: a state of the earliest level; mc_engine_read_states
 *              reads it), first_level its BFS level (1-based), trace_len the states of mc_engine_violation_trace.  An entry with
 *              states == 0 && outside > 0, and the fatal entry: the state that was being expanded.  UINT64_MAX / 0 / 0: nothing found.
 * mc_result's counters describe the search as far as it went: the complete graph when nothing fatal happened.
 * Two limits.  The PROPERTY of the Paxos family (MC_SPEC_PAXOS) is a property of a step, not of a state: it has
 * no row among the invariant entries; a step that breaks it ends the search and is the fatal entry (kind MC_V_INVARIANT, its index).
 * The snapshot-isolation lowering (MC_SPEC_SSI) evaluates, per stored state, the invariants its last step can have changed, which is
 * exact while every ancestor satisfied them: past a violator, a descendant that still breaks the same history invariant without
 * touching it again is not counted, so `states` of those invariants can be below TLC's count under -continue.  Its `find` predicate
 * and lock invariants are evaluated on every state.
 * mc_engine_violations: *n_inout capacity in, count out (MC_EBADCFG with the count when the buffer is too small).  MC_ESTATE on an
 * engine created without MC_F_CONTINUE.
 * mc_engine_violation_trace: mc_engine_trace's contract for entry k: the parent chain that ends in first_state; where the violator is
 * not stored (states == 0 && outside > 0) the chain of the smallest (parent, action slot) plus the successor rebuilt from it.
 * MC_ESTATE without the flag; MC_EBADCFG for k out of range or an entry with nothing to show. */
typedef struct {
    int32_t kind;             /* MC_V_INVARIANT, MC_V_DEADLOCK, or the fatal error's MC_V_ASSERT / MC_V_SPECERR / MC_V_INVARIANT     */
    int32_t invariant;        /* the index, or -1                                                           */
    uint64_t states, outside;
    uint64_t first_state;
    uint32_t first_level, trace_len;
} mc_violation;
typedef struct {
    uint32_t flagged_levels;  /* BFS levels (Init = level 1 included) after which a violation key was set  */
    uint32_t passes;          /* launches of the two kernels of engine_violations.h                        */
    uint32_t fatal;           /* 1: the LAST entry is the fatal error that ended the search                */
    uint32_t pad;
} mc_violations_info;
int mc_engine_violations(mc_engine *e, mc_violations_info *info, mc_violation *out, size_t *n_inout);
int mc_engine_violation_trace(mc_engine *e, size_t k, uint8_t *states_out, int32_t *actions_out, size_t *n_inout);
/* the name of INVARIANT `index` of a spec, as the reports print it ("?" when there is none) */
const char *mc_invariant_name(const mc_spec_desc *spec, int index);

/* ------------------------------------------------------------------ the state graph (TLC's `-dump dot`)
 * After a search the engine knows every state it found; mc_engine_graph adds how they connect: the edge list of the reachable graph in
 * CSR form, built on the device from the resident arena and seen-set, and kept there until the next search.  State i of the graph is
 * arena index i (mc_engine_read_states; state i + 1 of `-dump`); row i of dst[] / action[] is [offsets[i], offsets[i + 1]), in slot
 * order; action ids are mc_action_name's, the ones mc_engine_coverage lists.
 *   * A pair (expanded state, slot) that counts in mc_result.generated contributes: an edge to the state itself (a stuttering step);
 *     an edge to the stored state its successor is; or nothing but a count in `dropped` — a successor that is stored nowhere: a failed
 *     Assert, an evaluation error, a successor outside the CONSTRAINT, an invariant-breaking successor of a lowering that does not
 *     store those.  So  initial states generated + edges + dropped == mc_result.generated  for every model (the first term is
 *     mc_engine_coverage's generated[Init]).
 *   * The states with out-edges are the ones the search expanded — the levels mc_engine_coverage counts: up to max_levels /
 *     max_distinct, or to the end of the level that found a violation.  The unexpanded last level (the queue) has degree 0; so has a
 *     terminal state inside an expanded level.
 * mc_engine_graph is valid after any mc_engine_run / mc_engine_step that returned a result (ok, budget or a violation), needs no flag,
 * and changes nothing a following mc_engine_step computes.  MC_ESTATE before the first run, after mc_engine_simulate, and on a
 * restored engine that has not run yet; MC_EBADCFG on a sharded engine and for a search of 2^31 - 1 states or more (the scan's item
 * count); MC_EARENA (the byte count in mc_last_error) when the device has no room for it: 4 bytes per seen-set slot while it is built, then 8 bytes per state and 6 per edge.  A stored state or an
 * unflagged in-model successor that the seen-set does not hold fails the call with MC_ESTATE and builds no graph (mc_last_error names
 * the first such state and slot; two different states with one fingerprint are the only legitimate cause).  The next run / step /
 * simulate / restore releases the graph.
 * mc_engine_graph_read: the rows of states [first, first + count).  offsets_out: count + 1 entries, relative to offsets_out[0] = 0;
 * *nedges_inout: capacity of dst_out / action_out in, edges out (MC_EBADCFG with the count when they are too small).  MC_ESTATE
 * without a built graph. */
typedef struct {
    uint64_t states;        /* = mc_result.distinct of the search the graph belongs to         */
    uint64_t expanded;      /* states whose successors were generated (the rest: the queue)    */
    uint64_t init_states;   /* stored initial states: arena indices 0 .. init_states-1         */
    uint64_t edges;         /* entries of dst[] / action[]                                     */
    uint64_t self_loops;    /* of those, dst == src                                            */
    uint64_t dropped;       /* generated successors that are stored nowhere                    */
    uint32_t max_out_degree;
    uint32_t pad;
    double   seconds;       /* index + both passes, device work included                       */
} mc_graph_info;
int mc_engine_graph(mc_engine *e, mc_graph_info *out);
int mc_engine_graph_read(mc_engine *e, uint64_t first, uint64_t count, uint64_t *offsets_out /* count + 1 */, uint32_t *dst_out,
                         int32_t *action_out, size_t *nedges_inout);

/* ------------------------------------------------------------------ strongly connected components, and Termination under weak fairness
 * mc_engine_scc: the strongly connected components of the graph of mc_engine_graph (built first if it is not), found on the device by
 * trimming and forward colouring / backward reachability over the CSR arrays and their transpose.  Edges that end where they start
 * count for nothing: a state is a component of its own unless a cycle through ANOTHER state passes it.  The id of a component is the
 * least arena index among its states, so mc_engine_scc_read's array is a function of the graph alone.  Every lowering; the errors are
 * mc_engine_graph's.  Device memory beside the graph: 16 bytes per state and 4 per edge (MC_EARENA with the byte count).
 * mc_engine_liveness: does every behaviour of  Init /\ [][Next]_vars /\ \A p \in Fair : WF_vars(proc_p)  reach the state in which
 * all processes are Done (the translation's `Termination`)?  Fair = the process instances whose bit is set in weak_fair_mask (bit k =
 * instance k, in the order of the slots; mc_program_fairness gives the mask a program's `fair` keywords ask for).  Exact over the
 * COMPLETE graph: a component C is fair iff every fair process either takes a step u -> v, u # v, inside C or is disabled in some
 * state of C; the property is violated iff some fair component holds no Done state.  Compiled PlusCal
 * programs only (MC_ENOSPEC otherwise); MC_ESTATE unless the engine's last search finished without a violation and with an empty
 * queue; MC_EBADCFG on a sharded engine, and for a mask that names more instances than the program has.  1 byte per edge and 20 per
 * state more.
 * mc_engine_liveness_trace: the counterexample of the last violated check as arena indices (mc_engine_read_states turns them into
 * states).  prefix: a path of the graph from an initial state to the chosen component's least state — the fair component closest to
 * the initial states.  cycle: a closed walk inside the component from that state (cycle[0] == prefix[last]); the last entry has an
 * edge back to cycle[0]; for every fair process it takes a real step of the process or passes a state where it is disabled.  0 cycle
 * entries: the behaviour stutters for ever in prefix[last].  *n*_inout: capacities in, counts out (MC_EBADCFG with the counts when
 * too small).  Deterministic.  All of this is released where the graph is. */
typedef struct {
    uint64_t states;
    uint64_t components;       /* one-state components included                                      */
    uint64_t nontrivial;       /* components of more than one state                                  */
    uint64_t largest;          /* states of the largest component                                    */
    uint32_t trim_rounds;      /* sweeps launched, in batches of 8 (a batch that changes nothing ends a fixed point) */
    uint32_t colour_rounds;
    uint32_t backward_rounds;
    uint32_t passes;           /* trim + colouring passes that found some nontrivial component       */
    double   seconds;          /* transpose included, graph build excluded                           */
} mc_scc_info;
typedef struct {
    int32_t  violated;         /* 0: Termination holds, 1: violated                                  */
    uint32_t pad;
    uint64_t fair_components;  /* fair components without a Done state                               */
    uint64_t root;             /* the least id among them (valid when violated)                      */
    uint64_t root_size;        /* its number of states                                               */
    double   seconds;          /* per-edge processes, reduction and verdict (components excluded)    */
} mc_live_info;
int mc_engine_scc(mc_engine *e, mc_scc_info *out);
int mc_engine_scc_read(mc_engine *e, uint64_t first, uint64_t count, uint32_t *scc_out);
int mc_engine_liveness(mc_engine *e, uint64_t weak_fair_mask, mc_live_info *out);
int mc_engine_liveness_trace(mc_engine *e, uint32_t *prefix_out, size_t *nprefix_inout, uint32_t *cycle_out, size_t *ncycle_inout);

/* ------------------------------------------------------------------ <>Q, []<>Q, <>[]P and P ~> Q under weak fairness
 * A cfg PROPERTY of a compiled PlusCal program other than `Termination` names a definition of one of these four shapes over state
 * predicates, under bounded `\A`s and conjunctions; mc_program_live_property lists the checks it becomes (one per quantifier instance)
 * and the names the front end refused, with the reason.  The distinct predicates are compiled with the program and evaluated on demand:
 * mc_engine_predicates: bit k of bits_out[i] = predicate k in arena state first + i (built, with the graph, on first use; 4 bytes per
 * state; MC_ESTATE with the predicate and the least state where evaluating one fails).
 * mc_engine_liveness_check: one check, as a triple of state sets — M, where a violating suffix may stay; S, where it may be entered;
 * T, of which a state must recur:
 *     kind                          M        S                        T
 *     MC_LIVE_LEADS_TO    P ~> Q    ~Q       P /\ ~Q                  all
 *     MC_LIVE_INF_OFTEN   []<>Q     ~Q       ~Q                       all
 *     MC_LIVE_EVENTUALLY  <>Q       ~Q       initial states with ~Q   all
 *     MC_LIVE_STABLE      <>[]P     all      all                      ~P
 * violated iff some strongly connected component C of the graph induced by M (one-state components included) is fair — every fair
 * process takes a step u -> v, u # v, inside C or is disabled, IN THE FULL GRAPH, in some state of C —, holds a state of T and is
 * reachable inside M from a state of S that lies in M.  One component build per distinct M, kept while the graph lives; mc_engine_scc's
 * components are untouched.  witness: the least arena index among the S states from which such a component is reached; root: the
 * component the counterexample ends in (from the witness along strictly decreasing distance, the least successor each time).
 * mc_engine_liveness_trace then gives that counterexample: the prefix runs from an initial state through the witness to the first
 * state of the component, the cycle is a closed walk from there that meets the fairness condition by itself and, for MC_LIVE_STABLE,
 * passes the component's least ~P state.  Device memory beside mc_engine_liveness's: 4 bytes per state for the predicate bits, 4 for
 * the distances, 8 per distinct mask.  Errors: mc_engine_liveness's, and MC_EBADCFG for a predicate index the program does not
 * have, a refused property or an unknown kind. */
enum { MC_LIVE_LEADS_TO = 0, MC_LIVE_INF_OFTEN = 1, MC_LIVE_EVENTUALLY = 2, MC_LIVE_STABLE = 3 };
typedef struct mc_live_property {
    char    origin[64];        /* the cfg's PROPERTY name                                            */
    char    name[128];         /* of this check: origin, `.k` for conjunct k of several, `[i = v]`   */
    int32_t kind;              /* MC_LIVE_*; -1 when refused                                         */
    int32_t p, q;              /* predicate indices (P / Q of the table above), -1 = none            */
    int32_t refused;           /* 1: the front end does not check this name                          */
    char    reason[256];       /* why (refused)                                                      */
} mc_live_property;
typedef struct mc_live_check_info {
    int32_t  violated;
    uint32_t sweeps;           /* of the reach pass, in batches of 8                                 */
    uint64_t fair_components;  /* fair components of the masked graph that hold a T state            */
    uint64_t witness;          /* valid when violated: see above                                     */
    uint64_t root;
    uint64_t root_size;
    uint64_t mask_states;      /* states in M                                                        */
    uint64_t bad_starts;       /* S states from which a violating component is reached               */
    uint32_t scc_builds;       /* component builds this call needed (0: the mask's were kept)        */
    uint32_t pad;
    double   seconds;          /* everything the call did, component builds included                 */
} mc_live_check_info;
int mc_engine_predicates(mc_engine *e, uint64_t first, uint64_t count, uint32_t *bits_out);
int mc_engine_liveness_check(mc_engine *e, uint64_t weak_fair_mask, const mc_live_property *prop, mc_live_check_info *out);
/* the component ids the last mc_engine_liveness_check judged: those of the graph induced by its M (the least arena index of the state's
 * component; a state outside M is its own) — mc_engine_scc_read's array for MC_LIVE_STABLE.  MC_ESTATE without such a check. */
int mc_engine_liveness_components(mc_engine *e, uint64_t first, uint64_t count, uint32_t *scc_out);
/* ------------------------------------------------------------------ the same under strong fairness of whole processes
 * `fair+ process` asks for SF_vars(proc_p): a process that is enabled again and again must step.  weak_mask / strong_mask name the
 * weakly and the strongly fair instances (disjoint: SF implies WF; mc_program_fairness_strong gives a program's).  A set X of M that
 * is one state or strongly connected by its own edges is fair iff every weak process is taken inside X or disabled in some state of
 * X, and every strong process that is enabled in some state of X is taken inside X; a check is violated iff some fair X holds a T
 * state and is reachable inside M from an S state of M (Termination: M = all, S = the initial states, T = not Done).  Decided by
 * refinement: the components of the open states, each weakly unfair one closed, each one blocked by strong processes stripped of the
 * states that enable them, the rest found again, at most popcount(strong_mask) + 1 rounds.  With strong_mask == 0 every field of
 * mc_live_info / mc_live_check_info but `seconds` is the weak call's.  mc_engine_liveness_components and mc_engine_liveness_trace
 * serve the last check of either kind: after a strong one the refined ids (a final component's id where it was found, every other
 * state its own index) and a cycle inside one final component that takes a real step of every strong process taken in it.  Device
 * memory beside the weak calls': 25 bytes per state.  Errors: the weak twins', MC_EBADCFG for masks that overlap or name an instance
 * the program does not have, MC_ESTATE for a refinement that did not converge within its bound. */
typedef struct mc_live_strong_info {
    uint32_t rounds;            /* of the refinement (1: no component was blocked)                    */
    uint32_t scc_builds;        /* component builds of rounds >= 2 (never kept)                       */
    uint64_t closed_states;     /* states of M the refinement closed                                  */
    uint64_t final_components;  /* final violating components                                         */
    double   seconds;           /* the whole call                                                     */
} mc_live_strong_info;
int mc_engine_liveness_strong(mc_engine *e, uint64_t weak_mask, uint64_t strong_mask, mc_live_info *out, mc_live_strong_info *strong_out);
int mc_engine_liveness_check_strong(mc_engine *e, uint64_t weak_mask, uint64_t strong_mask, const mc_live_property *prop, mc_live_check_info *out,
                                    mc_live_strong_info *strong_out);
/* ------------------------------------------------------------------ fairness label by label
 * PlusCal's fairness is finer than "one process, one conjunct": a label `l:-` of a fair process is left out of its conjunct, a label
 * `l:+` gets a conjunct SF_vars(l(self)) of its own, and every procedure a fair process reaches gets one (the labels of the procedure's
 * copies in that process; the process's own conjunct is then over its own labels alone).  Two notions replace
 * "process instance" in the rule above.  A UNIT is the class of an edge: a function of the instance that steps and of the label at
 * pc[self] in the source state (at most 127).  A CONJUNCT is one WF_vars / SF_vars conjunct of the translation's Spec, a set of units
 * of one instance (at most 64); of_unit[u] has one bit per conjunct unit u belongs to — two for a `+` label of a weakly fair process,
 * none for a `-` label or a label of an unfair process.  weak_mask / strong_mask are masks of conjuncts.  The rule is the strong
 * calls' with "conjunct" for "process": an edge of unit u counts for the conjuncts of of_unit[u].  mc_program_fairness_units fills
 * the struct for a compiled program (returns the number of conjuncts; *refusal as mc_program_fairness: a VIEW, more than 64
 * conjuncts or 127 units — named with the count); mc_program_fairness_conjunct: conjunct k for its instance, as the translation prints it with the
 * instance's identifier for `self` (an identifier that is neither an integer nor written out in the process's set is shown as the
 * number the program keeps for it), NULL past the last.  The engine calls take the edges' units from the program (k_live_unit) and the table from *fu.  Errors: the strong
 * twins', and MC_EBADCFG for masks that overlap, a conjunct bit >= nconj in a mask or in of_unit[], nunits or nconj out of range or
 * nunits smaller than the program's units.  When every unit is one process instance, of_unit[u] = 1 << u and the masks are
 * mc_program_fairness_strong's, every field but `seconds` equals the strong calls'.  mc_engine_liveness_components and
 * mc_engine_liveness_trace serve the last check of any kind: after this one the cycle takes, for every weak conjunct, a real step
 * of it inside the component or passes a state where it is disabled, and a real step of every strong conjunct taken in the component. */
typedef struct mc_fair_units {
    int32_t  nunits, nconj;     /* units 0 .. nunits - 1 (<= 127), conjuncts 0 .. nconj - 1 (<= 64)    */
    uint64_t of_unit[128];      /* the conjuncts of every unit; 0 past nunits                         */
    uint64_t weak_mask;         /* the WF_vars conjuncts                                              */
    uint64_t strong_mask;       /* the SF_vars conjuncts (disjoint)                                   */
} mc_fair_units;
int mc_engine_liveness_units(mc_engine *e, const mc_fair_units *fu, mc_live_info *out, mc_live_strong_info *strong_out);
int mc_engine_liveness_check_units(mc_engine *e, const mc_fair_units *fu, const mc_live_property *prop, mc_live_check_info *out,
                                   mc_live_strong_info *strong_out);
/* the units of the edges [first_edge, first_edge + count) of mc_engine_graph_read's numbering, as the last check by units filled them
 * (-1: the terminating disjunct); MC_ESTATE without such a check */
int mc_engine_liveness_edge_units(mc_engine *e, uint64_t first_edge, uint64_t count, int8_t *unit_out);
/* copy `count` resident states starting at arena index `first` (discovery order: level by level)
 * to the host, mc_state_bytes() bytes each — TLC's "states/" dump, for tests and tooling */
int mc_engine_read_states(mc_engine *e, uint64_t first, uint64_t count, uint8_t *out);

/* ------------------------------------------------------------------ simulation (TLC's `-simulate [num=N] -depth D -seed S`)
 * Random walks from the initial states, one GPU lane per walk, no seen-set.  Walk w (0 <= w < num) is a function of
 * (seed, w, depth) alone: its initial state is init(H(seed, w) mod num_init); at each step every slot of the current state is
 * evaluated and checked as the BFS checks it, and the walk takes the enabled, in-model, non-stuttering successor whose slot has
 * the least H(seed, w, step, slot) (the lower slot on a tie); a successor equal to its parent counts as stuttering whether or not
 * the lowering marks it (the terminating disjunct of a PlusCal translation), and is passed over.  A walk ends at `depth` states, at its first violation, at a
 * deadlock, or when only out-of-model or stuttering successors are left (DESIGN.md "Simulation").  Walks run in rounds of a fixed
 * size, in index order; a run stops after the first round that holds a violation and reports its lowest-indexed violating walk,
 * whose counterexample mc_engine_trace then returns.  The same (seed, num, depth) on the same model gives the same result on any
 * device and with any engine capacities.  mc_engine_request_stop (from the progress callback, which is called after every launch with
 * (rounds done, generated, states reached, walks completed)) ends the run with MC_V_BUDGET; a stop inside a round reports no violation
 * of that round, whose lowest-indexed violating walk may not have ended yet.  A later mc_engine_run / mc_engine_step starts the BFS over. */
#define MC_SIM_END_DEPTH 1         /* the walk reached `depth` states                                          */
#define MC_SIM_END_VIOLATION 2     /* invariant, Assert, evaluation error, or deadlock with MC_F_DEADLOCK        */
#define MC_SIM_END_DEADLOCK 3      /* no enabled successor, deadlock checking off                               */
#define MC_SIM_END_OUT_OF_MODEL 4  /* every enabled successor violates a CONSTRAINT (or the initial state does) */
#define MC_SIM_END_STUTTER 5       /* only stuttering successors are left                                       */
#define MC_SIM_END_OVERFLOW 6      /* a fixed-capacity slot array overflowed (the call fails with MC_EOVERFLOW) */
#define MC_SIM_MAX_DEPTH 1000000
typedef struct {
    uint64_t num;             /* walks, at most 2^40; 0 = until a violation, mc_engine_request_stop or 2^40 walks */
    uint64_t seed;
    uint32_t depth;           /* states per walk at most (TLC's -depth, default 100), 1 .. MC_SIM_MAX_DEPTH  */
    uint32_t record;          /* K: record walks 0 .. K-1 into the arrays below (0 = none)                 */
    int32_t *record_slots;    /* K * depth: [k * depth + s] = slot from state s to state s + 1 of walk k, -1 past its end */
    uint32_t *record_len;     /* K: states walk k reached (0: it did not run)                               */
    uint32_t *record_end;     /* K: MC_SIM_END_* of walk k (0: it did not run)                              */
} mc_sim_opts;
typedef struct {
    uint64_t walks;           /* walks completed                                                           */
    uint64_t steps;           /* states reached, initial states included                                   */
    uint64_t generated;       /* successors evaluated (+ initial states): the BFS's "states generated" unit  */
    uint64_t violating_walk;  /* index of the walk the counterexample belongs to (verdict != MC_V_OK / BUDGET) */
    uint32_t max_depth;       /* states of the longest walk                                                */
    int32_t verdict;          /* MC_V_OK (num walks, no violation), MC_V_BUDGET (stopped), or the violation's */
    int32_t violated_invariant; /* as in mc_result                                                         */
    uint32_t trace_len;       /* states of the counterexample (mc_engine_trace), 0 if none                 */
    double seconds;
} mc_sim_result;
int mc_engine_simulate(mc_engine *e, const mc_sim_opts *opts, mc_sim_result *out);

/* ------------------------------------------------------------------ recorded behaviours against the model
 * "Is every one of these logged executions a behaviour of my spec?"  A behaviour is a sequence of observations o_0 .. o_{T-1}, T >= 1,
 * each a row of mc_state_bytes(spec) bytes in the layout mc_engine_read_states / mc_state_apply use (what an implementation logs: the
 * variables' cells).  One byte mask of the same width goes with the batch (NULL: everything is observed); a state s MATCHES o iff
 * (s ^ o) & mask == 0.  Candidate sets: K_0 = the initial states that match o_0; K_i = the distinct rows that match o_i and are a
 * successor — through an enabled slot — of a member of K_{i-1}; with MC_BEH_F_STUTTER also the members of K_{i-1} that match o_i
 * themselves (the stuttering step [Next]_vars allows).  A successor whose evaluation fails (Assert, evaluation error, a full slot array)
 * is no step and is counted in `errors`; one outside a CONSTRAINT is a step (a CONSTRAINT bounds the search, not the system) and is
 * counted in `outside` where it matches; invariants are not checked.  Distinct is by row, never by fingerprint (a VIEW).
 * One GPU wavefront decides one behaviour, one lane per candidate: a set that would pass MC_BEH_MAX_CANDIDATES rows makes the behaviour
 * MC_BEH_AMBIGUOUS — not decided; no candidate is ever dropped.  Every field of a verdict is a function of the behaviour, the mask and
 * the flags alone: not of the batch's order, the engine's capacities, `iters` or the device.
 * Refused (MC_EBADCFG + mc_last_error): an empty behaviour, a model with more than 65536 initial states, a sharded engine, and an
 * MC_F_JIT engine (its rows are packed and there is no way to import an interpreter's row into them).  The engine's search, if any,
 * is left as it is.
 * Unlogged steps: with MC_BEH_F_HIDDEN(H) in flags, up to H model steps that leave every observed cell unchanged may lie between
 * o_{i-1} and o_i (an implementation logs when something it shows changes; the model also steps through labels that move only pc or a
 * local).  K_i is then built from the closure C of K_{i-1}: K_{i-1} plus, depth by depth up to H, the distinct successors that still
 * match o_{i-1}.  Every member of C is evaluated once (`generated`); its successors join K_i where they match o_i.  A closure that would
 * pass MC_BEH_MAX_CANDIDATES rows makes the behaviour ambiguous like a K_i that does; `peak` covers the closures.  No hidden step comes
 * before o_0, and what follows the last observation does not matter.  H = 0 is the rule above, field for field. */
#define MC_BEH_ACCEPTED 1         /* K_{T-1} is not empty: step = T                                              */
#define MC_BEH_REJECTED 2          /* K_step is empty (step = 0: no initial state matches)                       */
#define MC_BEH_AMBIGUOUS 3         /* K_step would hold more than MC_BEH_MAX_CANDIDATES rows: not decided        */
#define MC_BEH_MAX_CANDIDATES 64
#define MC_BEH_MAX_INIT 65536
#define MC_BEH_F_STUTTER 1u        /* an observation may repeat the state before it                              */
#define MC_BEH_F_HIDDEN(h) (((h) & 0xffu) << 8)   /* up to h unlogged steps between two observations (flags bits 8..15) */
#define MC_BEH_MAX_HIDDEN 255
typedef struct {
    uint64_t count;           /* behaviours                                                                 */
    const uint64_t *first;    /* [count + 1]: behaviour b is observations first[b] .. first[b + 1] - 1 of rows */
    const uint8_t *rows;      /* first[count] rows of mc_state_bytes(spec) bytes                             */
    const uint8_t *mask;      /* mc_state_bytes(spec) bytes, or NULL                                         */
    uint32_t flags;           /* MC_BEH_F_*                                                                  */
    uint32_t iters;           /* observations a launch advances a behaviour by at most; 0 = the default (16) */
} mc_beh_opts;
typedef struct {
    int32_t verdict;          /* MC_BEH_*                                                                   */
    uint32_t step;            /* T (accepted), or the observation that decided                              */
    uint32_t candidates;      /* size of the last non-empty candidate set                                   */
    uint32_t peak;            /* size of the largest one                                                    */
    uint64_t generated;       /* initial states built + enabled successors evaluated, the deciding step included */
    uint64_t outside;         /* matching steps that leave the CONSTRAINTs                                  */
    uint64_t errors;          /* enabled successors that are no step: Assert, evaluation error, overflow    */
} mc_beh_verdict;
typedef struct {
    uint64_t accepted, rejected, ambiguous;
    uint64_t observations;    /* observations examined (a behaviour decided at `step` < T: step + 1)        */
    uint64_t generated;
    uint64_t first_rejected;  /* least index of a rejected behaviour, ~0 if none                            */
    double seconds;
} mc_beh_result;
int mc_engine_behaviours(mc_engine *e, const mc_beh_opts *opts, mc_beh_verdict *out, mc_beh_result *result);
/* Why: behaviour b once more, on the host, with parent links.  One model path s_0 .. s_{n-1} through its candidate sets: n = the
 * verdict's step (the whole behaviour if accepted; 0 if no initial state matches).  states_out: rows, slots_out[k]: the slot from
 * s_{k-1} to s_k (-1 for s_0, -2 for a stuttering step).  *n_inout: capacity in, n out (MC_EBADCFG with n when too small).  The path
 * is deterministic: it ends in the least row of the last set, and a row reached in several ways keeps the least slot. */
int mc_engine_behaviour_witness(mc_engine *e, const mc_beh_opts *opts, uint64_t b, uint8_t *states_out, int32_t *slots_out, size_t *n_inout);
/* The same with unlogged steps (MC_BEH_F_HIDDEN in opts->flags, which mc_engine_behaviour_witness refuses: its path has one state per
 * observation): obs_out[k] = the observation state k stands at; a hidden state repeats the index of the observation before it.
 * n <= (H + 1) * the verdict's step.  A closure member keeps the link of its least depth, then least slot, then least parent. */
int mc_engine_behaviour_path(mc_engine *e, const mc_beh_opts *opts, uint64_t b, uint8_t *states_out, int32_t *slots_out, uint32_t *obs_out,
                             size_t *n_inout);

/* Checkpoint / recover — TLC checkpoints a run into its states/ directory ("-- Checkpointing of run states/01-08-03-18-14-01
 * completed.", reference examples/SpecifyingSystems/AdvancedExamples/testout1:10; .gitignore:2) and continues it with -recover.
 * mc_engine_checkpoint: after an mc_engine_run that ended without a violation (normally MC_V_BUDGET), write every distinct
 *   state found (the arena's blocks as they lie in HBM), the level boundaries, the counters and — with MC_F_TRACE — the
 *   parent pointers to `path`.  The seen-set is not written.
 * mc_engine_restore: load such a file into an engine created for the SAME spec descriptor (MC_EBADCFG otherwise); the next
 *   mc_engine_run rebuilds the seen-set from the states' fingerprints and continues with the checkpoint's last level as
 *   the frontier: counters, depth, per-level counts and counterexamples are those of an uninterrupted run.  max_levels /
 *   max_distinct of the new engine are absolute (they count the checkpointed part).  Single-GPU engines only. */
int mc_engine_checkpoint(mc_engine *e, const char *path);
int mc_engine_restore(mc_engine *e, const char *path);
/* profiling aid: re-expand every resident state of the last run (all probes hit); extra_flags 16 = no probes */
int mc_engine_debug_reexpand(mc_engine *e, unsigned extra_flags, double *ms);
/* profiling builds only (libtlamc.so compiled with -DMC_PHASE_PROF, profiles/phase_prof.sh): shader-clock cycles per phase of the
 * by-family expand kernel summed over all wavefronts since the last reset (48 words: layout in engine.hip); MC_ESTATE otherwise */
int mc_engine_debug_phases(mc_engine *e, uint64_t *out48, int reset);
/* profiling only: set / clear bits of the engine's flags between two calls (the A/B and ablation bits a kernel reads at run time) — e.g. run
 * to a level normally, then time ONE more level (mc_engine_step) with an ablation bit on.  Never changes what a run without the bits computes. */
int mc_engine_debug_flags(mc_engine *e, uint32_t set, uint32_t clear);
/* read-only: the form of the engine's seen-set — its buckets and the slots of one (8, or 4 where the table is so much larger than the arena
 * that it can never be more than a third full); buckets * slots = table_capacity rounded up to whole 64-slot groups */
int mc_engine_seen_layout(mc_engine *e, uint64_t *buckets, uint32_t *slots);
void mc_engine_destroy(mc_engine *e);

/* ------------------------------------------------------------------ sharded (multi-GPU) step API
 * One engine per GPU / process; the seen-set is partitioned by fingerprint high bits
 * (owner = mc_fp_owner).  The caller (tla_rust_amd/sharded.py) moves the buckets between
 * ranks with an all-to-all over RCCL/xGMI; all pointers are device pointers it allocated.
 * Per level and per round:
 *   expand     : frontier chunk -> candidate fingerprints bucketed by owner
 *   (all-to-all of fingerprints)
 *   probe      : owner inserts received fingerprints, answers one byte (1 = new) per fingerprint
 *   (all-to-all of answers, reversed)
 *   materialise: sender builds the full successor state of every "new" answer, bucketed by owner
 *   (all-to-all of states)
 *   ingest     : owner appends received states to its next-level frontier.
 * Exchange format of full states: each owner's bucket is a whole number of 64-state BLOCKS
 * (mc_state_bytes() * 64 bytes each), word-major inside a block like the HBM arena, so both ends
 * move them with coalesced accesses; send_counts[] are STATES, a bucket occupies
 * ceil(count / 64) blocks.  mc_shard_ingest takes ONE source's bucket per call. */
/* Optional: hand the engine the HIP stream (hipStream_t) the caller issues its collectives on.  The engine then
 * enqueues bucket compaction, probe, keep, materialise and ingest on THAT stream and returns without waiting
 * (stream order ties them to the caller's all-to-alls); only calls that return counts to the host
 * (expand_finish, materialise, end_level, counters) block.  enable = 0 restores the blocking default.
 * With it mc_shard_keep* reports *n_new = 0: the count stays on the device until mc_shard_end_level. */
int mc_shard_set_stream(mc_engine *e, void *hip_stream, int enable);
int mc_shard_begin(mc_engine *e);                                  /* Init: keep the initial states this rank owns */
/* Alternative start: every rank runs the same single-GPU BFS until a level has at least min_frontier states (the
 * small first levels are not worth a collective each), keeps the states of that level whose fingerprint it owns as its
 * local frontier and holds all prefix fingerprints in its seen-set.  levels_out[0 .. *nlevels) = states per level of the
 * prefix, the last one being the level the sharded rounds continue with (*nlevels in: capacity, out: count).  Only
 * rank 0 reports the prefix's `generated`; distinct_local excludes what another rank already counts.  max_distinct /
 * max_levels (0 = none) are the budgets of the WHOLE job: the prefix stops where a single-GPU run would.
 * The level it stops at is the FIRST one with at least min_frontier states.  The rank's share lies behind the prefix in its arena
 * (indices sum(levels_out) ...), each entry a copy (mc_shard_fetch: parent_slot 0xfffc, parent_idx = the original). */
int mc_shard_begin_replicated(mc_engine *e, uint64_t min_frontier, uint64_t max_distinct, uint64_t max_levels,
                              uint64_t *levels_out, uint32_t *nlevels);
int mc_shard_level_size(mc_engine *e, uint64_t *frontier_states);  /* local frontier of the current level          */
int mc_shard_expand(mc_engine *e, uint64_t first, uint64_t count,  /* chunk of the local frontier                  */
                    uint64_t *send_fp, uint64_t send_cap, uint64_t *send_counts /* [shard_count] host */);
/* The same step split in two so that rounds can be software-pipelined: _launch enqueues the expand of a chunk
 * into `slot` (0 or 1) on the engine's main stream and returns at once; _finish waits for it and compacts the
 * slot's buckets into send_fp.  Between them the caller may run probe / keep / materialise / ingest for the
 * OTHER slot (they execute on the engine's side stream) and its collectives.  mc_shard_expand = both, slot 0. */
int mc_shard_expand_launch(mc_engine *e, uint32_t slot, uint64_t first, uint64_t count, uint64_t send_cap);
int mc_shard_expand_finish(mc_engine *e, uint32_t slot, uint64_t *send_fp, uint64_t send_cap, uint64_t *send_counts);
int mc_shard_probe(mc_engine *e, const uint64_t *recv_fp, uint64_t n, uint8_t *answers);
int mc_shard_materialise(mc_engine *e, const uint8_t *answers_back, uint8_t *send_states, uint64_t send_cap,
                         uint64_t *send_counts /* [shard_count] host, in states */);
/* answers_back: one byte per fingerprint of the slot's send_fp, same positions, non-zero = new.  Owner t's bucket holds the successors
 * of the positively answered positions of ITS range, in the order of those positions, and the lanes behind its last state are zero;
 * send_cap is in states.  Neither this call nor mc_shard_keep* consumes the slot's candidates: until the slot's next
 * mc_shard_expand_launch either may be called again with other answers. */
int mc_shard_materialise_slot(mc_engine *e, uint32_t slot, const uint8_t *answers_back, uint8_t *send_states,
                              uint64_t send_cap, uint64_t *send_counts);
int mc_shard_ingest(mc_engine *e, const uint8_t *recv_states, uint64_t n);
/* FIXED-CAPACITY rounds of the "stay" form — nothing in a round waits for the host: every rank sends every rank a bucket of
 * exactly `cap` words, word 0 = the number of fingerprints that follow (in band: no size message, no device-to-host copy
 * before the payload all-to-all can be sized), so the two collectives of a round are equal-split all-to-alls of cap words and
 * cap bytes per peer.
 *   _expand_pack(slot, send_fp[shard_count * cap], cap): after mc_shard_expand_launch(slot, ...) — orders itself behind the
 *       expand kernel with an event and packs owner t's candidates into send_fp[t * cap + 1 ...], count in send_fp[t * cap];
 *   _probe_pack(recv_fp[shard_count * cap], cap, answers[shard_count * cap]): bucket s came from rank s; answers keep the
 *       positions and are 0 outside a bucket's count;
 *   _keep_pack(slot, answers_back[shard_count * cap], cap): the sender materialises its positively answered candidates, appended
 *       to its frontier in the order of their positions.  answers_back must be 0 at every count word and behind every bucket's
 *       count (what _probe_pack writes there): no candidate lies at such a position, and a non-zero byte would be taken for one;
 *       the bucket of an owner that did not fit (count word 0) holds nothing;
 * cap must be the same on every rank (derive it from the level's frontier sizes, which every rank knows).  A bucket that
 * does not fit is not truncated: the level fails with MC_EROUTE at mc_shard_end_level ("an exchange bucket is full"). */
int mc_shard_expand_pack(mc_engine *e, uint32_t slot, uint64_t *send_fp, uint64_t cap);
int mc_shard_probe_pack(mc_engine *e, const uint64_t *recv_fp, uint64_t cap, uint8_t *answers);
int mc_shard_keep_pack(mc_engine *e, uint32_t slot, const uint8_t *answers_back, uint64_t cap);
/* device-side wait of the caller's stream for the slot's last keep: call it before a collective overwrites the answers
 * buffer that keep was given (a caller with one buffer per slot; callers that allocate per round need not) */
int mc_shard_wait_keep(mc_engine *e, uint32_t slot);
/* "stay" alternative to materialise + all-to-all + ingest: the positively answered candidates of the last
 * mc_shard_expand are materialised into THIS rank's frontier (only fingerprints crossed xGMI).  The caller
 * uses it once the frontier is large enough to stay balanced, and falls back to the moving form to rebalance. */
int mc_shard_keep(mc_engine *e, const uint8_t *answers_back, uint64_t *n_new);              /* slot 0 */
int mc_shard_keep_slot(mc_engine *e, uint32_t slot, const uint8_t *answers_back, uint64_t *n_new);
int mc_shard_end_level(mc_engine *e, uint64_t *new_local_states);  /* swap frontiers                                */
int mc_shard_counters(mc_engine *e, uint64_t *generated, uint64_t *distinct_local, int32_t *verdict);
/* Before a sharded run that stops on a budget reports: evaluate the invariants of this rank's unexpanded frontier for the
 * specs that check invariants when a state is expanded (the snapshot-isolation models); TLC checks a state when it is
 * generated, so no counted state may stay unchecked.  A violation shows up in mc_shard_counters' verdict.  No-op for the
 * other specs. */
int mc_shard_check_frontier(mc_engine *e);
/* Counterexamples of a sharded run (engines created with MC_F_TRACE): every state records the rank and arena index of its
 * parent.  A state that stays on the rank that generated it (stay mode, local-owner shortcut, replicated prefix) has a local
 * parent; a state that MOVES to its owner takes its parent with it: after mc_shard_materialise_slot the sender fills
 * `send_parents` (one word per moved state, same owner order, (index << 16) | slot), the caller exchanges it like the states,
 * and the owner calls mc_shard_ingest_parents right after the mc_shard_ingest of the same bucket.
 * mc_shard_violation: this rank's first violation (arena index, slot code as in the single-GPU engine: 0xffff deadlock,
 * 0xfffd the state itself violates an invariant, otherwise the slot whose successor does).
 * mc_shard_fetch: one step of the walk — the packed state at `idx` of this rank, the rank / index of its parent
 * (0xffffffff: an initial state) and the slot that produced it (0xfffc: this entry is a COPY of state parent_idx made by the
 * replicated prefix, not a step).  With bit 63 of `idx` set the low bits are an ORDINAL of Init's enumeration: the state is
 * rebuilt from it (an invariant violated by an initial state reports that ordinal, slot 0xfffe, not an arena index). */
int mc_shard_materialise_parents(mc_engine *e, uint32_t slot, uint64_t *send_parents);
int mc_shard_ingest_parents(mc_engine *e, const uint64_t *recv_parents, uint64_t n, uint32_t src_rank);
int mc_shard_violation(mc_engine *e, int32_t *found, uint64_t *idx, uint32_t *slot, int32_t *verdict, int32_t *invariant);
int mc_shard_fetch(mc_engine *e, uint64_t idx, uint8_t *state_out, uint32_t *parent_rank, uint64_t *parent_idx, uint32_t *parent_slot);
/* One checkpoint file per rank (TLC checkpoints a run and continues it with -recover: testout1:10 "-- Checkpointing of run
 * states/... completed."; mc_engine_checkpoint is the single-GPU form).  After an mc_shard_run* that ended without an error —
 * normally MC_V_BUDGET — every rank writes ITS share with mc_shard_checkpoint (a different path per rank): arena, parent
 * pointers (index, slot, rank), its seen-set slice as it lies in HBM (the states a rank holds are the ones it generated or
 * was sent, the fingerprints it stores are the ones it OWNS: the slice cannot be rebuilt from the arena), its counters and the
 * job's level table.  mc_shard_restore loads such a file into an engine created for the same spec, rank, world size,
 * table_capacity and MC_F_TRACE (MC_EBADCFG otherwise; arena_capacity may differ); the next mc_shard_run* of those engines
 * continues with the unexpanded frontier instead of starting at Init — every rank must have restored a file of the SAME run
 * (checked: MC_EBADCFG on all ranks otherwise).
 * mc_shard_note_levels / mc_shard_resume are the level loop's side of it (shard_loop.h): the loop leaves the job's level table
 * with the engine when a run ends, and asks a restored engine for it when the next one begins (*nlevels = 0: nothing restored). */
int mc_shard_checkpoint(mc_engine *e, const char *path);
int mc_shard_restore(mc_engine *e, const char *path);
int mc_shard_note_levels(mc_engine *e, const uint64_t *levels, uint32_t n, int32_t verdict);
int mc_shard_resume(mc_engine *e, uint64_t *levels_out, uint32_t *nlevels);

/* ------------------------------------------------------------------ hip-rccl back-end (tla_rust_amd/csrc/shard_rccl.cpp)
 * The level loop of the sharded search behind the C ABI, collectives over RCCL (xGMI): one process per GPU, no Python.
 *   rank 0:      mc_comm_unique_id(id)            -- ncclGetUniqueId; ship the MC_COMM_ID_BYTES to the other ranks (file, socket, env ...)
 *   every rank:  mc_comm_create(id, rank, world, device, &c)          -- ncclCommInitRank + the stream the collectives run on
 *                mc_engine_create(spec, cfg with shard_rank / shard_count, &e)
 *                mc_shard_run(e, c, &opts, &result)                    -- the whole search; every rank gets the global counters
 * replaces: TLC's worker pool ("Number of worker threads", examples/serializableSnapshotIsolation.tla:52-53) scaled past one
 * device.  Per level one collective for frontier sizes + verdicts + statuses (ncclAllGather); the rounds inside a level are
 * ncclSend / ncclRecv groups — of exact sizes after a small all-gather of the bucket counts (the default), or the fixed-capacity
 * exchanges above (mc_shard_*_pack, no host wait inside a level): MC_SHARD_* below.  Any RCCL failure returns MC_ERCCL
 * (mc_last_error() carries ncclGetErrorString).  A rank-local failure (a full exchange bucket, MC_ETABLEFULL, MC_EOVERFLOW,
 * an allocation) does not leave the others waiting in a collective: every rank's status travels with the per-level
 * all-gather and all ranks leave the loop together with the first failing rank's code.  Levels whose new states STAY where they
 * were generated need 9 bytes per routed candidate (the expand of round r+1 overlaps the exchange, the probes and the
 * materialisation of round r; the fixed-capacity forms also overlap the exchange of round r+1 with the probes of round r and move
 * their buckets whole); small or unbalanced levels MOVE the new states to
 * their owners (mc_shard_materialise_slot / mc_shard_ingest).  `mc X.tla -gpus P` is this API with forked ranks. */
#define MC_COMM_ID_BYTES 128
typedef struct mc_comm mc_comm;
#define MC_SHARD_NO_PREFIX 1u /* mc_shard_opts.flags: shard from Init on (mc_shard_begin) instead of the replicated prefix */
/* How a STAY level exchanges its candidates (mc_shard_opts.flags; `mc -gpus P -exchange exact | measured | packed`):
 *   default (neither flag): HOST-PACED rounds with exact sizes — the ranks exchange their P bucket counts (one small all-gather),
 *     then all_to_all_v moves exactly 8 bytes per routed candidate out and 1 byte back: the least the exchange can move, no
 *     capacity to guess and no bucket that could overflow, for one host wait + two small all-gathers per round (the counts, and "every
 *     rank has the buffers its announced sizes need": a rank that could not allocate must not leave its peers inside the all-to-all;
 *     one agreement covers both all-to-alls of the round) (the next round's expand is
 *     launched before them and overlaps the exchange, the probes and the materialisation of this one);
 *   MC_SHARD_PACKED: pipelined FIXED-CAPACITY rounds, counts in band, no host wait inside a level (mc_shard_*_pack); the buckets are
 *     moved whole, so their capacity is the exchange volume: it is sized from the previous level's MEASURED fill
 *     (the loop reads the in-band counts of every round back, asynchronously; cap_safety_pct) ...
 *   MC_SHARD_PACKED | MC_SHARD_FIXED_CAPS: ... or from packed_fanout alone (rounds 2-3).  A search restarted after MC_EROUTE in a
 *     measured level runs so. */
#define MC_SHARD_FIXED_CAPS 2u
#define MC_SHARD_PACKED 4u
/* what one rank's level loop did (diagnostics; filled when mc_shard_opts.stats != NULL).  With TLAMC_SHARD_DEBUG set in the
 * environment rank 0 also prints one line per level to stderr: its kind, states, rounds, the fullest bucket per expanded state. */
typedef struct {
    uint64_t replicated_levels; /* levels every rank ran itself (mc_shard_begin_replicated)                                  */
    uint64_t stay_levels;       /* levels whose new states stayed on the generating rank (9 B per candidate cross xGMI)      */
    uint64_t move_levels;       /* levels whose new states moved to their owner (small frontiers, rebalancing)               */
    uint64_t rounds;            /* exchange rounds (one chunk per rank each)                                                 */
    uint64_t sent_bytes;        /* bytes THIS rank handed to the all-to-alls for other ranks (fingerprints, answers, states) */
    uint64_t distinct_local;    /* states resident on this rank at the end (its share)                                       */
    uint64_t max_frontier;      /* over the sharded levels: largest max-over-ranks frontier ...                              */
    uint64_t mean_frontier;     /* ... and the mean frontier of that same level (imbalance = max / mean)                     */
    uint64_t restarts;          /* times the search was started over from Init with twice the fan-out allowance (MC_EROUTE)  */
    uint64_t routed_candidates; /* candidates THIS rank sent to other ranks' seen-set slices (stay rounds: the in-band counts; move
                                 * rounds: the exact sizes): 9 bytes each (fingerprint out, answer back) is what the exchange needs */
    uint64_t fp_answer_bytes;   /* the part of sent_bytes that carried fingerprints and answers (the rest: moved states, parents)  */
    uint64_t measured_levels;   /* stay levels whose buckets were sized from the previous level's measured fill                   */
    uint64_t engine_ns;         /* host time this rank spent inside engine calls (mc_shard_*: launches AND the waits for its own streams) */
    uint64_t collective_ns;     /* host time inside the transport's collectives (the exchange itself + waiting for the slowest peer)  */
    uint64_t collectives;       /* how many collectives that was                                                                  */
} mc_shard_stats;
typedef struct {
    uint64_t chunk_states;    /* frontier states per round and rank (0 = 2^19); clamped to the engine's chunk_states         */
    uint64_t max_distinct;    /* budgets of the whole job (0 = none)                                                        */
    uint64_t max_levels;
    uint64_t replicate_until; /* states per rank a level must have before the search is sharded (0 = 2^15); below it every
                               * rank runs the same fused BFS (mc_shard_begin_replicated)                                    */
    uint64_t packed_fanout;   /* in-model successors per expanded state the fixed-capacity buckets allow for (0 = 16); a
                               * round that exceeds it is never truncated: the level fails on every rank (MC_EROUTE) and
                               * mc_shard_run* starts the search over with twice the allowance (at most 5 times)            */
    uint64_t stay_threshold;  /* states per rank a level needs before its new states STAY where they were generated
                               * (0 = 2^15); smaller levels MOVE every new state to its owner, which is what spreads a
                               * small frontier over the ranks                                                              */
    double rebalance_ratio;   /* a level whose largest per-rank frontier exceeds ratio x the mean is a MOVE level again:
                               * a drifting rank cannot stall the level loop (0 = 1.25)                                     */
    uint64_t move_fanout;     /* in-model successors per expanded state the buffers of a move round allow for (0 = 32)      */
    uint32_t flags;           /* MC_SHARD_*                                                                                 */
    uint32_t cap_safety_pct;  /* a stay level's buckets hold this many percent of what the previous level's fullest bucket held
                               * per expanded state (0 = 140; never more than packed_fanout allows; the first stay level and a level
                               * after one without packed rounds use packed_fanout).  Only the capacity — i.e. the bytes moved over
                               * xGMI — depends on it, never a count: a bucket that does not fit still fails the level (MC_EROUTE)   */
    mc_shard_stats *stats;    /* NULL or where to put this rank's loop statistics                                            */
} mc_shard_opts;
/* TEST-ONLY hooks of this part of the library (a one-GPU lab has no second device): the environment variable TLAMC_RCCL names the
 * file dlopen()ed instead of /opt/rocm/lib/librccl.so (tests/_fakerccl: the nine nccl* entry points over POSIX shared memory, so
 * that P ranks can share ONE device — RCCL itself refuses two ranks on a device); `mc X.tla -gpus P -samedevice` and
 * `bench.py --gpus N --share-gpu` put every rank on device 0 for it.  None of them belongs in a deployment: without TLAMC_RCCL
 * the real RCCL is loaded, and a run through the stand-in says so in its report / bench line ("NOT_A_MEASUREMENT").
 * TLAMC_TEST_FAIL_AT = "rank:level:code[,rank:level:code...]" makes that rank of mc_shard_run* fail that BFS level with that status,
 * once per process (tests/test_sharded_gloo.py: two DIFFERENT failures in one level must end every rank with ONE agreed code —
 * MC_EROUTE, i.e. a restart, only if every failing rank reports MC_EROUTE). */
int mc_comm_unique_id(uint8_t id_out[MC_COMM_ID_BYTES]);
int mc_comm_create(const uint8_t id[MC_COMM_ID_BYTES], uint32_t rank, uint32_t world, int32_t device, mc_comm **out);
void mc_comm_destroy(mc_comm *c);
/* host-side all-gather of `bytes` bytes per rank over the communicator (rank r's block at all_out + r * bytes): a barrier,
 * a max-over-ranks of wall times, the shares of a run — what a multi-process host needs besides the search itself */
int mc_comm_all_gather(mc_comm *c, const void *mine, void *all_out, uint64_t bytes);
int mc_shard_run(mc_engine *e, mc_comm *c, const mc_shard_opts *opts, mc_result *out);
/* Counterexample of a sharded run that ended in a violation (engines created with MC_F_TRACE): the behaviour is walked back
 * parent by parent ACROSS the ranks' arenas (mc_shard_violation / mc_shard_fetch on the rank that holds the state, one small
 * all-gather per step).  Collective: every rank calls it and receives the same trace.  states_out: *n_inout records of
 * mc_state_bytes() bytes (capacity in, count out), first the initial state; slots_out[k] = the action slot that led from state
 * k-1 to state k (-1 for k = 0): mc_state_action(spec, state k-1, slot) names it.  *final_slot >= 0: the violation is an
 * INVARIANT broken by a successor that is stored nowhere — the caller appends mc_state_apply(spec, last state, *final_slot);
 * -1 otherwise (Assert / evaluation error / deadlock / the last state itself violates).  *n_inout = 0: no rank found one. */
int mc_shard_trace(mc_engine *e, mc_comm *c, uint8_t *states_out, int32_t *slots_out, size_t *n_inout, int32_t *final_slot);

/* ---- bring your own collectives.  mc_shard_run / mc_shard_trace are written against this table; mc_comm fills it with RCCL
 * (ncclSend / ncclRecv groups, ncclAllGather).  A host that already owns a communicator — torch.distributed's process group
 * (tla_rust_amd/sharded.py: backend "nccl" = RCCL, or gloo staged through the host in the CPU tests), MPI — hands its own
 * functions over and gets the SAME level loop.  All buffers the loop passes to all_to_all / all_to_all_v come from alloc()
 * (device memory for a HIP engine) and are passed by their base address; every collective is ordered on `hip_stream` like a
 * kernel launch (the loop makes that stream wait for its producers with events and lets its consumers wait for it), may
 * return before it has completed, and must be called by every rank in the same order.  Return 0 or a negative MC_E* code. */
typedef struct mc_transport {
    void *user;
    uint32_t rank, world;
    void *hip_stream;  /* hipStream_t the collectives are ordered on; NULL: the collectives are synchronous host calls */
    void *(*alloc)(void *user, size_t bytes);
    void (*release)(void *user, void *p);
    /* equal split: bytes_per_peer bytes at send + p * bytes_per_peer go to rank p, rank p's block lands at recv + p * bytes_per_peer */
    int (*all_to_all)(void *user, const void *send, void *recv, uint64_t bytes_per_peer);
    /* variable split: send_bytes[p] bytes at send + send_off[p] go to rank p; recv_bytes[p] bytes from rank p land at recv + recv_off[p] */
    int (*all_to_all_v)(void *user, const void *send, const uint64_t *send_off, const uint64_t *send_bytes, void *recv,
                        const uint64_t *recv_off, const uint64_t *recv_bytes);
    /* HOST buffers, blocking: rank r's `bytes` bytes appear at all_out + r * bytes on every rank */
    int (*all_gather)(void *user, const void *mine, void *all_out, uint64_t bytes);
    /* OPTIONAL (may be NULL: a transport zero-initialises the struct and fills what it has): all_to_all without the rank's own
     * block — recv + rank * bytes_per_peer is left untouched.  The fingerprint exchange of a stay round uses it when present: a
     * rank's own bucket is empty by construction (candidates it owns are probed where they are generated), so moving it is a
     * device copy of the whole bucket for its count word; the loop zeroes that word itself. */
    int (*all_to_all_others)(void *user, const void *send, void *recv, uint64_t bytes_per_peer);
} mc_transport;
int mc_comm_transport(mc_comm *c, mc_transport *out);  /* the RCCL functions of a communicator; valid while c lives */
int mc_shard_run_transport(mc_engine *e, const mc_transport *t, const mc_shard_opts *opts, mc_result *out);
int mc_shard_trace_transport(mc_engine *e, const mc_transport *t, uint8_t *states_out, int32_t *slots_out, size_t *n_inout,
                             int32_t *final_slot);
/* what the level loop needs to know about an engine: its expand stream (the loop orders bucket compaction / its collectives
 * against it with events), the largest chunk one launch takes, whether parent pointers are kept (MC_F_TRACE) */
int mc_shard_info(mc_engine *e, void **main_stream_out, uint64_t *chunk_states_out, int32_t *traced_out);

/* ------------------------------------------------------------------ PlusCal front-end (host only)
 * The reference's workflow is `pcal2tla *tla` then `tlc *tla` (Makefile:3-7).  mc_pcal_translate is the first
 * half: it returns the module text with the TLA+ translation of its `--algorithm` inserted (p-manual.pdf App. B).
 * mc_program_compile is what lets the checker run a PlusCal spec nobody hand-lowered: the algorithm (p- or c-syntax;
 * labels, := , if/elsif/else, while, either/or, with, await/when, assert, skip, goto, define, macros, LET; integers, booleans, strings,
 * functions over constant sets, bounded sequences and arrays of them, sets of small naturals; procedures incl. recursion, records incl. nested
 * ones, sequences and sets of records: DESIGN.md section 9) becomes a bytecode program every GPU lane interprets on its own packed state
 * (tla_rust_amd/csrc/spec_vm.h).  Two bounds come from the environment at compile time: $TLAMC_PCAL_SEQ, the element cells per sequence /
 * set of records (1 .. 16, default 8; a longer one is MC_EOVERFLOW, never truncated), and $TLAMC_PCAL_STACK, the frames per recursive
 * procedure (default 4; a deeper call fails an assertion at the call).  cfg_text: CONSTANT(S) with integer / string / model-value / set values and
 * INVARIANT(S) naming zero-argument definitions of the module; NULL = no constants, no invariants. */
typedef struct mc_program mc_program;
int mc_pcal_translate(const char *tla_text, char *out, size_t cap);   /* >= 0: bytes needed (NUL excluded); < 0: MC_E* */
int mc_program_compile(const char *tla_text, const char *cfg_text, mc_program **out);
int mc_program_spec(const mc_program *p, mc_spec_desc *out);          /* valid while p lives */
const char *mc_program_translated(const mc_program *p);               /* the module text after translation */
/* the program as generated C++ (a header for tla_rust_amd/csrc/spec_gen.h: what MC_F_JIT compiles): the text's length, at most cap - 1
 * characters of it in buf; MC_EBADCFG (+ mc_last_error) when the program uses an instruction the translator does not cover */
long mc_program_codegen(const mc_program *p, char *buf, size_t cap);
const char *mc_program_invariant(const mc_program *p, int index);     /* name of INVARIANT number index */
int mc_program_assert_pos(const mc_program *p, int index, int *line, int *col);  /* source position of an assert */
/* fairness of the algorithm: *weak_fair_mask = the process instances declared `fair` (or all of them, `--fair algorithm`), bit k =
 * instance k in slot order; returns the number of instances.  *refusal (either may be NULL): NULL when mc_engine_liveness decides
 * `Termination` for this program, else the reason it cannot (`fair+`, a `+` / `-` label in a fair process, procedures). */
int mc_program_fairness(const mc_program *p, uint64_t *weak_fair_mask, const char **refusal);
/* the same for the strong calls: *strong_mask = the `fair+` instances, *weak_mask = the other fair ones (disjoint); *refusal is NULL
 * for a program whose only obstacle was `fair+`, and mc_program_fairness's words for everything else */
int mc_program_fairness_strong(const mc_program *p, uint64_t *weak_mask, uint64_t *strong_mask, const char **refusal);
/* the same label by label (mc_fair_units, above): pcal2tla's conjuncts for `fair+`, `+` / `-` labels and procedures */
int mc_program_fairness_units(const mc_program *p, mc_fair_units *out, const char **refusal);
const char *mc_program_fairness_conjunct(const mc_program *p, int k);
/* mc_program_translated with Spec's fairness conjuncts written label by label, as pcal2tla writes them (the same text for a program
 * without `+` / `-` labels in fair processes) */
const char *mc_program_translated_labelfair(const mc_program *p);
/* the cfg's PROPERTY / PROPERTIES names, in cfg order; NULL past the last (what a caller that runs the search itself — `mc -gpus` —
 * must name as NOT checked) */
const char *mc_program_property(const mc_program *p, int index);
/* the checks (and refusals) the cfg's PROPERTY names other than Termination become, in cfg order: MC_OK, or MC_EBADCFG past the last.
 * mc_program_live_predicate: the text of predicate number index (with the quantifier values it was compiled for), NULL past the last */
int mc_program_live_property(const mc_program *p, int index, mc_live_property *out);
const char *mc_program_live_predicate(const mc_program *p, int index);
/* the cfg's VIEW and ACTION_CONSTRAINTs as the program honours them: the text of the view's definition ("<<x, pc>>"), NULL without a VIEW;
 * the name of action constraint number index (cfg order), NULL past the last.  With a view the fingerprint of a state is that of its view
 * values; which state represents a view value is the one that arrived first — reproducible exactly when equal views imply equal futures. */
const char *mc_program_view(const mc_program *p);
const char *mc_program_action_constraint(const mc_program *p, int index);
/* the SAFETY parts of the cfg's PROPERTYs that the search itself checks, one entry per conjunct, MC_EBADCFG past
 * the last.  MC_APROP_STEP: `[][A]_v`, evaluated as `A \/ UNCHANGED v` on every successor the search generates — new or seen before,
 * inside the model or not, refused by an ACTION_CONSTRAINT or not; never on the terminating disjunct or on a successor that is an
 * error already.  MC_APROP_ALWAYS: `[]P`, one more invariant behind the cfg's INVARIANTs.  MC_APROP_INIT: a state predicate beside a
 * `[][A]_v` (the shape Init /\ [][Next]_v /\ fairness), checked on the initial states.  A violation is MC_V_INVARIANT with
 * mc_result.violated_invariant = `index`: the `[]P` entries count among the invariants (mc_invariant_name gives the PROPERTY's name),
 * a step's and an initial predicate's index lies behind them, which is how a caller tells a property of a step from an invariant.
 * A successor that breaks an INVARIANT as well reports the invariant: the status word carries one index.  Under MC_F_CONTINUE a step
 * that breaks a `[][A]_v` is fatal, as the Paxos models' PROPERTY is: the search ends at the end of that level, the entry comes last. */
enum { MC_APROP_STEP = 0, MC_APROP_ALWAYS = 1, MC_APROP_INIT = 2 };
typedef struct mc_action_property {
    char    origin[64];        /* the cfg's PROPERTY name                                            */
    int32_t kind;              /* MC_APROP_*                                                         */
    int32_t index;             /* the invariant index a violation reports                            */
    char    text[256];         /* the conjunct as the module writes it, tokens joined by one blank   */
} mc_action_property;
int mc_program_action_property(const mc_program *p, int index, mc_action_property *out);
/* which bytes of a row a log of the named variables observes (mc_beh_opts.mask): `variables` = comma-separated names of the program's
 * variables; a record stands for its fields; `bytes` = mc_state_bytes of the program's descriptor.  MC_EBADCFG for an unknown name. */
int mc_program_observe(const mc_program *p, const char *variables, uint8_t *mask_out, size_t bytes);
void mc_program_free(mc_program *p);

/* ------------------------------------------------------------------ helpers (host only) */
size_t mc_state_bytes(const mc_spec_desc *spec);                    /* W, 0 if the spec is invalid   */
uint32_t mc_fp_owner(uint64_t fp, uint32_t shard_count);
/* canonical TLA+ text of one packed state ("/\ var = value" lines, README.md:272-276) */
int mc_state_format(const mc_spec_desc *spec, const uint8_t *state, char *buf, size_t cap);
const char *mc_action_name(const mc_spec_desc *spec, int32_t action);
/* host evaluation of one (packed state, slot) pair: the action id of the slot (for mc_action_name; negative MC_E* on error)
 * and the successor it produces — what a host needs to print a counterexample it assembled itself (sharded runs) */
int mc_state_action(const mc_spec_desc *spec, const uint8_t *state, int32_t slot);
int mc_state_apply(const mc_spec_desc *spec, const uint8_t *state, int32_t slot, uint8_t *successor_out);
/* the inverse of mc_state_format for MC_SPEC_PCAL (MC_ENOSPEC for the other lowerings): the text `mc -dump` / a TLC trace prints for one
 * state -> its row.  Conjuncts may be missing: a variable the text does not mention is unobserved — its cells are zero in row_out and
 * clear in mask_out (mc_state_bytes(spec) bytes each; mask_out may be NULL), the mentioned ones' are 0xff, as mc_program_observe gives
 * them.  MC_EPARSE (+ mc_last_error) for a text that is no state of the program: an unknown variable, a value of the wrong shape, a
 * string the program does not know. */
int mc_state_parse(const mc_spec_desc *spec, const char *text, uint8_t *row_out, uint8_t *mask_out);
const char *mc_strerror(int code);
const char *mc_last_error(void);                                    /* detail of the last failure    */
int mc_device_count(void);

/* ------------------------------------------------------------------ front-end
 * Replaces TLC's reading of X.cfg (grammar: examples/SpecifyingSystems/TLC/ConfigFileGrammar.tla:4-32)
 * and its selection of Init/Next/invariants; the spec itself is selected by MODULE name
 * (pcal_intro.tla:1) from the registry of hand-lowered specs. */
typedef struct mc_cfg mc_cfg;
int mc_cfg_parse(const char *text, size_t len, mc_cfg **out);
void mc_cfg_free(mc_cfg *c);
/* JSON rendering of the parsed cfg, for bindings and tests */
int mc_cfg_json(const mc_cfg *c, char *buf, size_t cap);
/* resolve module + cfg to a lowering; fails with MC_ENOSPEC for modules that are not lowered */
int mc_spec_resolve(const char *module_name, const mc_cfg *c, mc_spec_desc *out);
/* the front half of `tlc X.tla` (reference Makefile:6-7, README.md:262,356): read X.tla and the X.cfg beside it (or cfg_path),
 * pick the lowering (verified against the module text) or compile the PlusCal algorithm, and return the descriptor
 * mc_engine_create takes — what a multi-GPU host needs to create one engine per rank (mc_shard_*).  flags: MC_F_GENERIC.
 * *prog_out = the compiled program when the module went through the PlusCal compiler (the descriptor points into it: free
 * it with mc_program_free after the engines are destroyed), NULL otherwise. */
int mc_resolve_files(const char *tla_path, const char *cfg_path, unsigned flags, mc_spec_desc *out, mc_program **prog_out);
/* `tlc X.tla` end to end: read X.tla / X.cfg, run on `cfg->device`, write TLC's report text.
 * A TLA+ module that belongs to none of the lowered families (no PlusCal algorithm, not raft / the snapshot-isolation specs /
 * Voting / Paxos or a wrapper of them) is evaluated on the HOST by the general evaluator (csrc/tlaeval.cpp: the Specifying Systems
 * examples of the reference; `MCInnerSerial.tla` gives testout2:260-266): out->host_evaluated = 1, the report's first line says
 * so, cfg->max_levels / max_distinct / MC_F_DEADLOCK / MC_F_PROGRESS apply, $TLA_PATH (a ':'-separated list) names more module
 * directories.  A module of a lowered family is never evaluated on the host: what its lowering refuses stays MC_ENOSPEC. */
int mc_check_files(const char *tla_path, const char *cfg_path, const mc_config *cfg, char *report,
                   size_t report_cap, mc_result *out);
/* the same, and every distinct state found is written to dump_path in TLC's `-dump` layout ("State k:" + the
 * variables, blank line), in discovery order; dump_path NULL = mc_check_files */
int mc_check_files_dump(const char *tla_path, const char *cfg_path, const mc_config *cfg, char *report,
                        size_t report_cap, mc_result *out, const char *dump_path);
/* the same with TLC's -recover / checkpointing: recover_path (or NULL) is restored before the run, checkpoint_path (or
 * NULL) is written after a run that ended without an error; the report then carries TLC's line
 * "-- Checkpointing of run <path> completed." (testout1:10) */
int mc_check_files_ckpt(const char *tla_path, const char *cfg_path, const mc_config *cfg, char *report, size_t report_cap,
                        mc_result *out, const char *dump_path, const char *recover_path, const char *checkpoint_path);
/* mc_check_files, and the state graph is written to dot_path in TLC's `-dump dot[,actionlabels][,colorize]` layout: "strict digraph
 * DiskGraph", one node per state labelled with its text (initial states filled), one line per edge of mc_engine_graph, with
 * MC_DOT_ACTIONLABELS the action's name on it, with MC_DOT_COLORIZE a colour per action and a legend.  Node k is arena index k - 1:
 * the state `-dump` prints as "State k:".  The report gains "The state graph has <states> states and <edges> transitions (<self_loops>
 * self loops)." after the depth line.  Refused where mc_check_files_dump is (a module evaluated on the host, a cfg without a behaviour).
 * mc_check_files_dumps: both files from ONE search, so that they number the states alike (either path may be NULL), with
 * mc_check_files_ckpt's recover_path / checkpoint_path (or NULL): a recovered search that has run has its seen-set again, so its
 * graph — checkpointed levels included — is built like any other.  A dot file that cannot be written completely is removed. */
#define MC_DOT_ACTIONLABELS 1u
#define MC_DOT_COLORIZE 2u
int mc_check_files_dot(const char *tla_path, const char *cfg_path, const mc_config *cfg, char *report, size_t report_cap,
                       mc_result *out, const char *dot_path, unsigned dot_flags);
int mc_check_files_dumps(const char *tla_path, const char *cfg_path, const mc_config *cfg, char *report, size_t report_cap,
                         mc_result *out, const char *dump_path, const char *dot_path, unsigned dot_flags, const char *recover_path,
                         const char *checkpoint_path);
/* `mc X.tla -simulate`: the module and its cfg resolved as mc_check_files resolves them, then mc_engine_simulate with `opts`; the report
 * (seed, the error and its behaviour as in mc_check_files, "The number of states generated: G", the walks and the longest one) goes
 * to `report`.  A module without a GPU lowering is refused (MC_ENOSPEC).  *interrupt (optional; a SIGINT handler's flag) stops the
 * simulation between two launches: the report then says so (MC_V_BUDGET). */
int mc_simulate_files(const char *tla_path, const char *cfg_path, const mc_config *cfg, const mc_sim_opts *opts, char *report, size_t report_cap,
                      mc_sim_result *out, const volatile int *interrupt);
/* `mc X.tla -behaviours FILE [-observe v1,v2,...] [-stutter] [-hidden H]`: the module resolved as mc_check_files resolves it (a compiled PlusCal
 * program: the file's states are texts, mc_state_parse), FILE read — states as `mc -dump` / a TLC trace prints them, optional
 * "State k:" headers ignored, a blank line between states, a line of ---- between behaviours — and mc_engine_behaviours run on it.
 * observe: comma-separated variable names (mc_program_observe), or NULL: the variables every state of the file mentions.  flags:
 * MC_BEH_F_*.  The report gives the counts, a warning that names the ambiguous behaviours, and for the first rejected behaviour
 * "Error: Behaviour b is not a behaviour of the model: no step leads to observation i.", the witness in TLC's layout and the
 * observation.  With MC_BEH_F_HIDDEN(H) the first line says "up to H unlogged steps between observations", the error "no step, and no
 * step after up to H unlogged ones, leads to observation i", and the witness (mc_engine_behaviour_path) marks the states the log does
 * not have with "(not logged)".  Behaviours and observations are counted from 1 in the report. */
int mc_check_behaviours_files(const char *tla_path, const char *cfg_path, const mc_config *cfg, const char *behaviours_path, const char *observe,
                              unsigned flags, char *report, size_t report_cap, mc_beh_result *out);

#ifdef __cplusplus
}
#endif
#endif
