//! Rust host side of the C ABI in `include/tlamc.h` — the "Rust host over a thin C-ABI FFI" that
//! `BASELINE.json:north_star` asks for (the reference's README.md:12-16 planned a Rust implementation
//! checked with quickcheck).  NOT COMPILED IN THIS REPOSITORY'S CI: the build image has no Rust toolchain;
//! this file is the literal transcription of the header a maintainer would start from.
#![allow(non_camel_case_types)]
use std::ffi::{CStr, CString};
use std::os::raw::{c_char, c_int};

pub const MC_SPEC_ATOMIC_ADD: u32 = 1;
pub const MC_SPEC_PCAL_INTRO: u32 = 2;
pub const MC_SPEC_RAFT: u32 = 3;
pub const MC_SPEC_SSI: u32 = 4;
pub const MC_SPEC_PCAL: u32 = 5; // a PlusCal algorithm compiled by mc_program_compile
pub const MC_SPEC_PAXOS: u32 = 6; // examples/Paxos/Voting.tla, Paxos.tla under MCVoting / MCPaxos (+ .cfg)
pub const MC_F_GENERIC: u32 = 128;
pub const MC_F_DEADLOCK: u32 = 1;
pub const MC_F_TRACE: u32 = 2;
pub const MC_F_JIT: u32 = 262144; // MC_SPEC_PCAL: the compiled program as generated code, built for the device when the engine is created
pub const MC_DOT_ACTIONLABELS: u32 = 1; // mc_check_files_dot: the action name on every edge
pub const MC_DOT_COLORIZE: u32 = 2;     // ... and a colour per action, with a legend
pub const MC_F_CONTINUE: u32 = 67108864; // TLC's -continue: search on past violated invariants and deadlocks (mc_engine_violations); implies MC_F_TRACE, one-GPU engines only
pub const MC_F_COVERAGE: u32 = 16777216; // TLC's -coverage: per-action counts (mc_engine_coverage); implies MC_F_TRACE, one-GPU engines only
pub const MC_MAX_LEVELS: usize = 4096;

#[repr(C)]
pub struct mc_spec_desc { pub spec_id: u32, pub nparams: u32, pub params: [i64; 16] }
#[repr(C)]
pub struct mc_config {
    pub device: i32, pub flags: u32, pub table_capacity: u64, pub arena_capacity: u64, pub chunk_states: u64,
    pub max_levels: u64, pub max_distinct: u64, pub shard_rank: u32, pub shard_count: u32,
}
#[repr(C)]
pub struct mc_result {
    pub distinct: u64, pub generated: u64, pub queue_left: u64, pub depth: u32, pub verdict: i32,
    pub violated_invariant: i32, pub trace_len: u32, pub levels: u32, pub host_evaluated: u32, pub unchecked_properties: u32, pub seconds: f64,
    pub level_distinct: [u64; MC_MAX_LEVELS],
}
// simulation mode (TLC's -simulate num=N -depth D -seed S): mc_engine_simulate, mc_simulate_files
pub const MC_SIM_END_DEPTH: u32 = 1;
pub const MC_SIM_END_VIOLATION: u32 = 2;
pub const MC_SIM_END_DEADLOCK: u32 = 3;
pub const MC_SIM_END_OUT_OF_MODEL: u32 = 4;
pub const MC_SIM_END_STUTTER: u32 = 5;
pub const MC_SIM_END_OVERFLOW: u32 = 6;
pub const MC_SIM_MAX_DEPTH: u32 = 1000000;
#[repr(C)]
pub struct mc_sim_opts {
    pub num: u64, pub seed: u64, pub depth: u32, pub record: u32,
    pub record_slots: *mut i32, pub record_len: *mut u32, pub record_end: *mut u32,
}
#[repr(C)]
pub struct mc_sim_result {
    pub walks: u64, pub steps: u64, pub generated: u64, pub violating_walk: u64, pub max_depth: u32, pub verdict: i32,
    pub violated_invariant: i32, pub trace_len: u32, pub seconds: f64,
}
// recorded behaviours against the model (mc_engine_behaviours): rows are mc_state_bytes(spec) bytes each, `first` has count + 1 offsets
// into them, `mask` (same width, or null: everything is observed) says which bytes the log records
pub const MC_BEH_ACCEPTED: i32 = 1;
pub const MC_BEH_REJECTED: i32 = 2;
pub const MC_BEH_AMBIGUOUS: i32 = 3;
pub const MC_BEH_MAX_CANDIDATES: u32 = 64;
pub const MC_BEH_MAX_INIT: u64 = 65536;
pub const MC_BEH_F_STUTTER: u32 = 1;
pub const MC_BEH_MAX_HIDDEN: u32 = 255;
/// flags bits 8..15: up to `h` model steps that change no observed cell may lie between two observations
pub const fn mc_beh_f_hidden(h: u32) -> u32 { (h & 0xff) << 8 }
#[repr(C)]
pub struct mc_beh_opts {
    pub count: u64, pub first: *const u64, pub rows: *const u8, pub mask: *const u8, pub flags: u32, pub iters: u32,
}
#[repr(C)]
pub struct mc_beh_verdict {
    pub verdict: i32, pub step: u32, pub candidates: u32, pub peak: u32, pub generated: u64, pub outside: u64, pub errors: u64,
}
#[repr(C)]
pub struct mc_beh_result {
    pub accepted: u64, pub rejected: u64, pub ambiguous: u64, pub observations: u64, pub generated: u64, pub first_rejected: u64,
    pub seconds: f64,
}
// one entry of mc_engine_coverage: action id (-1 = Init), the states it was first to find, the successors it generated
#[repr(C)]
pub struct mc_action_coverage { pub action: i32, pub pad: u32, pub distinct: u64, pub generated: u64 }
// one entry of mc_engine_violations (an engine created with MC_F_CONTINUE): per INVARIANT index, then deadlock, then the fatal error; 40 bytes.
// first_state = u64::MAX: nothing found
#[repr(C)]
pub struct mc_violation {
    pub kind: i32, pub invariant: i32, pub states: u64, pub outside: u64, pub first_state: u64, pub first_level: u32, pub trace_len: u32,
}
#[repr(C)]
pub struct mc_violations_info { pub flagged_levels: u32, pub passes: u32, pub fatal: u32, pub pad: u32 } // fatal = 1: the last entry ended the search
// what mc_engine_graph built: the state graph of the last search in CSR form (rows by arena index); 64 bytes
#[repr(C)]
pub struct mc_graph_info {
    pub states: u64, pub expanded: u64, pub init_states: u64, pub edges: u64, pub self_loops: u64, pub dropped: u64,
    pub max_out_degree: u32, pub pad: u32, pub seconds: f64,
}
#[repr(C)]
pub struct mc_scc_info {
    pub states: u64, pub components: u64, pub nontrivial: u64, pub largest: u64,
    pub trim_rounds: u32, pub colour_rounds: u32, pub backward_rounds: u32, pub passes: u32, pub seconds: f64,
}
#[repr(C)]
pub struct mc_live_info { pub violated: i32, pub pad: u32, pub fair_components: u64, pub root: u64, pub root_size: u64, pub seconds: f64 }
#[repr(C)]
pub struct mc_live_strong_info { pub rounds: u32, pub scc_builds: u32, pub closed_states: u64, pub final_components: u64, pub seconds: f64 }
// one check a cfg's PROPERTY name became (mc_program_live_property), and what mc_engine_liveness_check* report about it
#[repr(C)]
pub struct mc_live_property { pub origin: [c_char; 64], pub name: [c_char; 128], pub kind: i32, pub p: i32, pub q: i32, pub refused: i32, pub reason: [c_char; 256] }
// one safety part of a cfg's PROPERTY (mc_program_action_property): kind 0 `[][A]_v`, 1 `[]P`, 2 an initial predicate
#[repr(C)]
pub struct mc_action_property { pub origin: [c_char; 64], pub kind: i32, pub index: i32, pub text: [c_char; 256] }
#[repr(C)]
pub struct mc_live_check_info { pub violated: i32, pub sweeps: u32, pub fair_components: u64, pub witness: u64, pub root: u64, pub root_size: u64,
                                pub mask_states: u64, pub bad_starts: u64, pub scc_builds: u32, pub pad: u32, pub seconds: f64 }
// fairness label by label: of_unit[u] = the WF / SF conjuncts unit u (an edge's class: instance and label of the source state) belongs to
#[repr(C)]
pub struct mc_fair_units { pub nunits: i32, pub nconj: i32, pub of_unit: [u64; 128], pub weak_mask: u64, pub strong_mask: u64 }
#[repr(C)]
pub struct mc_engine { _private: [u8; 0] }
#[repr(C)]
pub struct mc_program { _private: [u8; 0] }

extern "C" {
    pub fn mc_engine_create(spec: *const mc_spec_desc, cfg: *const mc_config, out: *mut *mut mc_engine) -> c_int;
    pub fn mc_engine_run(e: *mut mc_engine, out: *mut mc_result) -> c_int;
    pub fn mc_engine_step(e: *mut mc_engine, levels: u32, out: *mut mc_result) -> c_int;
    pub fn mc_engine_request_stop(e: *mut mc_engine) -> c_int;
    pub fn mc_engine_simulate(e: *mut mc_engine, opts: *const mc_sim_opts, out: *mut mc_sim_result) -> c_int;
    // one verdict per behaviour of the batch; behaviour_witness: behaviour b once more on the host, one model path through its
    // candidate sets (slots[k]: the slot into state k, -1 for the first, -2 for a stuttering step); *n_inout: capacity in, states out
    pub fn mc_engine_behaviours(e: *mut mc_engine, opts: *const mc_beh_opts, out: *mut mc_beh_verdict, result: *mut mc_beh_result) -> c_int;
    pub fn mc_engine_behaviour_witness(e: *mut mc_engine, opts: *const mc_beh_opts, b: u64, states: *mut u8, slots: *mut i32,
                                       n_inout: *mut usize) -> c_int;
    // the witness with the unlogged steps in it (mc_beh_f_hidden in opts.flags, which behaviour_witness refuses): obs[k] = the
    // observation state k stands at, a hidden state repeats the one before it; at most (h + 1) * step states
    pub fn mc_engine_behaviour_path(e: *mut mc_engine, opts: *const mc_beh_opts, b: u64, states: *mut u8, slots: *mut i32, obs: *mut u32,
                                    n_inout: *mut usize) -> c_int;
    pub fn mc_engine_trace(e: *mut mc_engine, states: *mut u8, actions: *mut i32, n_inout: *mut usize) -> c_int;
    // entries for Init and every action of the model, in action-id order; *n_inout: capacity in, count out
    pub fn mc_engine_coverage(e: *mut mc_engine, out: *mut mc_action_coverage, n_inout: *mut usize) -> c_int;
    // everything a search under MC_F_CONTINUE found; violation_trace: mc_engine_trace's contract for entry k
    pub fn mc_engine_violations(e: *mut mc_engine, info: *mut mc_violations_info, out: *mut mc_violation, n_inout: *mut usize) -> c_int;
    pub fn mc_engine_violation_trace(e: *mut mc_engine, k: usize, states: *mut u8, actions: *mut i32, n_inout: *mut usize) -> c_int;
    pub fn mc_invariant_name(spec: *const mc_spec_desc, index: c_int) -> *const c_char;
    // the state graph, built on the device after a search and kept until the next one; graph_read: the rows of states
    // [first, first + count): count + 1 offsets relative to the first, *nedges_inout capacity in / edges out
    pub fn mc_engine_graph(e: *mut mc_engine, out: *mut mc_graph_info) -> c_int;
    pub fn mc_engine_graph_read(e: *mut mc_engine, first: u64, count: u64, offsets_out: *mut u64, dst_out: *mut u32, action_out: *mut i32,
                                nedges_inout: *mut usize) -> c_int;
    // strongly connected components of that graph (scc[i] = the least arena index of state i's component) and `Termination` under weak
    // fairness of the process instances in the mask (compiled PlusCal programs; include/tlamc.h)
    pub fn mc_engine_scc(e: *mut mc_engine, out: *mut mc_scc_info) -> c_int;
    pub fn mc_engine_scc_read(e: *mut mc_engine, first: u64, count: u64, scc_out: *mut u32) -> c_int;
    pub fn mc_engine_liveness(e: *mut mc_engine, weak_fair_mask: u64, out: *mut mc_live_info) -> c_int;
    pub fn mc_engine_liveness_trace(e: *mut mc_engine, prefix_out: *mut u32, nprefix_inout: *mut usize, cycle_out: *mut u32,
                                    ncycle_inout: *mut usize) -> c_int;
    // the same under strong fairness of the instances in strong_mask (`fair+ process`), weak fairness of those in weak_mask
    pub fn mc_engine_liveness_strong(e: *mut mc_engine, weak_mask: u64, strong_mask: u64, out: *mut mc_live_info,
                                     strong_out: *mut mc_live_strong_info) -> c_int;
    // the same under pcal2tla's conjuncts label by label (`+` / `-` labels, `fair+`): the table from mc_program_fairness_units
    pub fn mc_engine_liveness_units(e: *mut mc_engine, fu: *const mc_fair_units, out: *mut mc_live_info, strong_out: *mut mc_live_strong_info) -> c_int;
    pub fn mc_engine_liveness_check_units(e: *mut mc_engine, fu: *const mc_fair_units, prop: *const mc_live_property, out: *mut mc_live_check_info,
                                          strong_out: *mut mc_live_strong_info) -> c_int;
    pub fn mc_engine_liveness_edge_units(e: *mut mc_engine, first_edge: u64, count: u64, unit_out: *mut i8) -> c_int;
    pub fn mc_program_translated_labelfair(p: *const mc_program) -> *const c_char;
    pub fn mc_program_fairness_units(p: *const mc_program, out: *mut mc_fair_units, refusal: *mut *const c_char) -> c_int;
    pub fn mc_program_fairness_conjunct(p: *const mc_program, k: c_int) -> *const c_char;
    pub fn mc_engine_read_states(e: *mut mc_engine, first: u64, count: u64, out: *mut u8) -> c_int;
    // TLC's checkpoint / -recover (testout1:10): write / reload the states found so far; the next run continues
    pub fn mc_engine_checkpoint(e: *mut mc_engine, path: *const c_char) -> c_int;
    pub fn mc_engine_restore(e: *mut mc_engine, path: *const c_char) -> c_int;
    pub fn mc_engine_destroy(e: *mut mc_engine);
    // one checkpoint file per rank of a sharded run (include/tlamc.h: mc_shard_checkpoint / mc_shard_restore)
    pub fn mc_shard_checkpoint(e: *mut mc_engine, path: *const c_char) -> c_int;
    pub fn mc_shard_restore(e: *mut mc_engine, path: *const c_char) -> c_int;
    // X.tla + X.cfg -> the descriptor mc_engine_create takes (one engine per rank in sharded mode)
    pub fn mc_resolve_files(tla: *const c_char, cfg_path: *const c_char, flags: u32, out: *mut mc_spec_desc,
                            prog_out: *mut *mut mc_program) -> c_int;
    pub fn mc_check_files(tla: *const c_char, cfg_path: *const c_char, cfg: *const mc_config, report: *mut c_char,
                          cap: usize, out: *mut mc_result) -> c_int;
    // TLC's -dump dot[,actionlabels][,colorize]: mc_check_files, and the state graph goes to dot_path (node k = State k of the plain
    // dump); _dumps: both dumps from one search, with mc_check_files_ckpt's recover / checkpoint paths (any of the paths may be null)
    pub fn mc_check_files_dot(tla: *const c_char, cfg_path: *const c_char, cfg: *const mc_config, report: *mut c_char, report_cap: usize,
                              out: *mut mc_result, dot_path: *const c_char, dot_flags: u32) -> c_int;
    pub fn mc_check_files_dumps(tla: *const c_char, cfg_path: *const c_char, cfg: *const mc_config, report: *mut c_char, report_cap: usize,
                                out: *mut mc_result, dump_path: *const c_char, dot_path: *const c_char, dot_flags: u32,
                                recover_path: *const c_char, checkpoint_path: *const c_char) -> c_int;
    pub fn mc_check_behaviours_files(tla: *const c_char, cfg_path: *const c_char, cfg: *const mc_config, behaviours_path: *const c_char,
                                     observe: *const c_char, flags: u32, report: *mut c_char, cap: usize, out: *mut mc_beh_result) -> c_int;
    // the inverse of mc_state_format for a compiled PlusCal program: row and mask (may be null) of mc_state_bytes(spec) bytes
    pub fn mc_state_parse(spec: *const mc_spec_desc, text: *const c_char, row_out: *mut u8, mask_out: *mut u8) -> c_int;
    pub fn mc_simulate_files(tla: *const c_char, cfg_path: *const c_char, cfg: *const mc_config, opts: *const mc_sim_opts,
                             report: *mut c_char, cap: usize, out: *mut mc_sim_result, interrupt: *const c_int) -> c_int;
    // PlusCal front-end: `pcal2tla` and the compiler to the GPU interpreter (include/tlamc.h)
    pub fn mc_pcal_translate(tla_text: *const c_char, out: *mut c_char, cap: usize) -> c_int;
    pub fn mc_program_compile(tla_text: *const c_char, cfg_text: *const c_char, out: *mut *mut mc_program) -> c_int;
    pub fn mc_program_spec(p: *const mc_program, out: *mut mc_spec_desc) -> c_int;
    pub fn mc_program_translated(p: *const mc_program) -> *const c_char;
    pub fn mc_program_codegen(p: *const mc_program, buf: *mut c_char, cap: usize) -> std::os::raw::c_long;
    pub fn mc_program_invariant(p: *const mc_program, index: c_int) -> *const c_char;
    // fairness of the algorithm (bit k of the mask: process instance k is weakly fair; *refusal: why Termination cannot be checked, or
    // null; returns the number of instances) and the cfg's PROPERTY names (null past the last)
    pub fn mc_program_fairness(p: *const mc_program, weak_fair_mask: *mut u64, refusal: *mut *const c_char) -> c_int;
    pub fn mc_program_fairness_strong(p: *const mc_program, weak_mask: *mut u64, strong_mask: *mut u64, refusal: *mut *const c_char) -> c_int;
    pub fn mc_program_property(p: *const mc_program, index: c_int) -> *const c_char;
    // the byte mask (mc_beh_opts.mask) of a log that records the named variables (comma-separated) only
    pub fn mc_program_observe(p: *const mc_program, variables: *const c_char, mask_out: *mut u8, bytes: usize) -> c_int;
    // the cfg's VIEW (the text of its definition, null without one) and ACTION_CONSTRAINT names (null past the last)
    pub fn mc_program_view(p: *const mc_program) -> *const c_char;
    pub fn mc_program_action_constraint(p: *const mc_program, index: c_int) -> *const c_char;
    // the safety parts of the cfg's PROPERTYs the search checks (`[][A]_v`, `[]P`, initial predicates): entry `index`, MC_EBADCFG past the last
    pub fn mc_program_action_property(p: *const mc_program, index: c_int, out: *mut mc_action_property) -> c_int;
    pub fn mc_program_free(p: *mut mc_program);
    pub fn mc_state_bytes(spec: *const mc_spec_desc) -> usize;
    pub fn mc_state_format(spec: *const mc_spec_desc, state: *const u8, buf: *mut c_char, cap: usize) -> c_int;
    pub fn mc_action_name(spec: *const mc_spec_desc, action: i32) -> *const c_char;
    pub fn mc_strerror(code: c_int) -> *const c_char;
    pub fn mc_last_error() -> *const c_char;
    pub fn mc_device_count() -> c_int;
}

#[derive(Debug)]
pub struct Outcome { pub distinct: u64, pub generated: u64, pub depth: u32, pub verdict: i32, pub host_evaluated: bool,
                     /// cfg PROPERTIES with a liveness part that were NOT checked (named in the report's "Warning:" line)
                     pub unchecked_properties: u32, pub report: String }

/// `tlc X.tla` (reference Makefile:6-7) from Rust.
pub fn check(tla: &std::path::Path, device: i32) -> Result<Outcome, String> {
    let path = CString::new(tla.to_str().ok_or("non-UTF-8 path")?).map_err(|e| e.to_string())?;
    let cfg = mc_config { device, flags: MC_F_DEADLOCK | MC_F_TRACE, table_capacity: 1 << 26, arena_capacity: 1 << 24,
                          chunk_states: 0, max_levels: 0, max_distinct: 0, shard_rank: 0, shard_count: 1 };
    let mut res: Box<mc_result> = unsafe { Box::new(std::mem::zeroed()) };
    let mut buf = vec![0u8; 1 << 20];
    let rc = unsafe { mc_check_files(path.as_ptr(), std::ptr::null(), &cfg, buf.as_mut_ptr() as *mut c_char, buf.len(), &mut *res) };
    if rc != 0 {
        return Err(unsafe { CStr::from_ptr(mc_last_error()) }.to_string_lossy().into_owned());
    }
    let end = buf.iter().position(|&b| b == 0).unwrap_or(0);
    Ok(Outcome { distinct: res.distinct, generated: res.generated, depth: res.depth, verdict: res.verdict, host_evaluated: res.host_evaluated != 0, unchecked_properties: res.unchecked_properties,
                 report: String::from_utf8_lossy(&buf[..end]).into_owned() })
}

#[cfg(test)]
mod tests {
    /// What the README's tutorial promises once the labels A:/B: are removed (README.md:349-352).
    #[test]
    fn committed_pcal_intro_has_no_error() {
        let o = super::check(std::path::Path::new("../../specs/pcal_intro.tla"), 0).unwrap();
        assert_eq!((o.verdict, o.distinct, o.generated, o.depth), (0, 3800, 5850, 5));
    }
}
