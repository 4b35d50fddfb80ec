"""Simulation mode on the GPU (mc_engine_simulate, k_simulate in tla_rust_amd/csrc/engine_sim.h): the device's walk w is the host's walk w
(tests/_simshim: the same sim_walk.h) for every family of lowerings, the interpreter and generated code walk alike, runs repeat exactly,
violations come with valid counterexamples, walks go deeper than the BFS does on the five-server raft model, and `mc -simulate` reports
like `tlc -simulate`."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

import helpers
import simwalk

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MC = ROOT / "tla_rust_amd" / "_build" / "mc"
SMALL = dict(table_capacity=1 << 16, arena_capacity=1 << 14, chunk_states=1 << 12)
SOUP = ROOT / "specs" / "pluscal" / "two_phase_soup.tla"
CAS = ROOT / "specs" / "pluscal" / "cas_counter.tla"


@pytest.fixture(scope="module")
def amd():
    import tla_rust_amd
    assert tla_rust_amd.device_count() >= 1, "no HIP device visible"
    return tla_rust_amd


def host_walks(spec, params, seed, n, depth, deadlock=True):
    h = simwalk.walks(spec, params, seed=seed, n=n, depth=depth, deadlock=deadlock)
    return [dict(len=w["len"], end=simwalk.END[w["end"]], slots=w["slots"]) for w in h["walks"]], h


def same_as_host(amd, spec, dev_params, host_params, seed, n, depth, deadlock=True, **kw):
    eng = amd.Engine(spec, dev_params, deadlock=deadlock, **SMALL, **kw)
    r = eng.simulate(n, depth, seed, record=n)
    eng.close()
    walks, h = host_walks(spec, host_params, seed, n, depth, deadlock)
    assert r.recorded == walks
    assert (r.walks, r.steps, r.generated, r.max_depth) == (h["walks_done"], h["steps"], h["generated"], h["max_depth"])
    assert r.violating_walk == (None if h["viol"] is None else simwalk.key_walk(h["viol"]))
    return r


FAMILIES = [
    ("atomic_add", [3], 40), ("pcal_intro", [1, 0, 20, 2], 40), ("raft", [2, 2, 2, 9, 1, 1], 60),
    ("raft", [3, 4, 2, 3, 1, 1, 10, 1, 4, 10], 100), ("ssi", [2, 2, 127, 0], 60), ("paxos", [0, 3, 2, 3, 15, 3, 1], 60),
]


@pytest.mark.parametrize("spec,params,depth", FAMILIES, ids=[f"{s}{p}" for s, p, _ in FAMILIES])
def test_device_walks_are_host_walks(amd, spec, params, depth):
    r = same_as_host(amd, spec, params, params, seed=2024, n=1000, depth=depth, deadlock=spec != "paxos")
    assert r.steps > 1000


def compiled(amd, path, cfg_path, invariants, constants):
    prog = amd.Program(path.read_text(), cfg_path.read_text())
    host = helpers.ShimProgram(path.read_text(), invariants=invariants, constants=constants)
    return prog, host


def test_interpreter_and_generated_code_walk_as_the_host(amd):
    prog, host = compiled(amd, CAS, ROOT / "specs" / "pluscal" / "cas_counter.cfg", ["NeverTooMany", "SeenIsOld"], {"Workers": 2, "N": 2})
    try:
        a = same_as_host(amd, "pcal", prog.params, host.params, seed=5, n=500, depth=50)
        b = same_as_host(amd, "pcal", prog.params, host.params, seed=5, n=500, depth=50, jit=True)
        assert {k: v for k, v in a.items() if k != "seconds"} == {k: v for k, v in b.items() if k != "seconds"}
    finally:
        prog.close()
        host.close()


def test_runs_repeat_and_do_not_depend_on_capacities(amd):
    params = [3, 4, 2, 3, 1, 1, 10, 1, 4, 10]
    keys = ("walks", "steps", "generated", "max_depth", "verdict", "trace_len", "violating_walk")
    outs = []
    for caps in (SMALL, SMALL, dict(table_capacity=1 << 20, arena_capacity=1 << 18, chunk_states=1 << 16)):
        eng = amd.Engine("raft", params, **caps)
        r = eng.simulate(300000, 60, 77)
        outs.append(({k: r[k] for k in keys}, eng.trace()))
        eng.close()
    assert outs[0] == outs[1] == outs[2]
    assert outs[0][0]["walks"] == 300000 and outs[0][0]["verdict"] == "ok"


def raw_trace(amd, eng, spec, params):
    L = amd.lib()
    W = L.mc_state_bytes(C.byref(amd.binding.spec_desc(spec, params)))
    cap = C.c_size_t(4096)
    states = C.create_string_buffer(W * cap.value)
    acts = (C.c_int32 * cap.value)()
    assert L.mc_engine_trace(eng._h, states, acts, C.byref(cap)) == 0
    return [states.raw[k * W:(k + 1) * W] for k in range(cap.value)], list(acts[:cap.value])


def check_violation(amd, spec, dev_params, host_params, verdict, num=100000, depth=100, seed=1, deadlock=True, invariant=None):
    eng = amd.Engine(spec, dev_params, deadlock=deadlock, **SMALL)
    r = eng.simulate(num, depth, seed)
    assert r.verdict == verdict and r.trace_len >= 1, dict(r)
    if invariant is not None:
        assert r.violated_invariant == invariant
    rows, acts = raw_trace(amd, eng, spec, dev_params)
    named = eng.trace()
    eng.close()
    assert len(rows) == r.trace_len and acts[0] == -1 and named[0][0] == "Initial predicate"
    # the host's walk of the same index: its slots rebuild the device's trace state by state (mc_state_apply, the product's host code)
    h = simwalk.walks(spec, host_params, seed=seed, n=1, depth=depth, first=r.violating_walk, deadlock=deadlock)
    slots = h["walks"][0]["slots"] + ([simwalk.key_slot(h["viol"])] if len(rows) > h["walks"][0]["len"] else [])
    assert len(slots) == len(rows) - 1 and h["walks"][0]["end"] == 2
    for k in range(1, len(rows)):
        assert amd.binding.state_apply(spec, dev_params, rows[k - 1], slots[k - 1]) == rows[k], k
    # no walk of a lower index of the round violates anything
    before = simwalk.walks(spec, host_params, seed=seed, n=min(r.violating_walk, 20000), depth=depth, deadlock=deadlock)
    assert before["viol"] is None or r.violating_walk == 0
    return r


def test_readme_model_violation_and_trace(amd):
    check_violation(amd, "pcal_intro", [1, 0, 20, 2], [1, 0, 20, 2], "assert")


def test_paxos_negative_control_violation(amd):
    check_violation(amd, "paxos", [0, 3, 2, 2, 15, 0, 3], [0, 3, 2, 2, 15, 0, 3], "invariant", deadlock=False, invariant=2)


def test_hasty_two_phase_soup_violation(amd):
    cfg = ROOT / "specs" / "pluscal" / "two_phase_soup_hasty.cfg"
    prog, host = compiled(amd, SOUP, cfg, ["Consistent", "OneDecision", "PreparedWereSent", "KnownMessages"], {"RM": 3, "Hasty": True})
    try:
        r = check_violation(amd, "pcal", prog.params, host.params, "invariant", num=20000, depth=40)
        assert r.violated_invariant == 0   # Consistent
    finally:
        prog.close()
        host.close()


def test_voting_deadlock_only_with_deadlock_checking(amd):
    params = [1, 3, 2, 2, 1, 3, 1]
    check_violation(amd, "paxos", params, params, "deadlock", num=2000, depth=100)
    eng = amd.Engine("paxos", params, deadlock=False, **SMALL)
    r = eng.simulate(2000, 100, 1, record=50)
    eng.close()
    assert r.verdict == "ok" and r.walks == 2000 and "deadlock" in {w["end"] for w in r.recorded}


def test_raft5_walks_deeper_than_the_bfs(amd):
    """config 4's model (5 servers): the BFS stops at 18 levels; a simulation at depth 100 reaches past them (with the default
    capacities of the packed state's slot arrays: bench.py's, sized for 18 levels, overflow deeper)"""
    eng = amd.Engine("raft", [5, 6, 2, 5, 1, 1], **SMALL)
    r = eng.simulate(20000, 100, 3)
    eng.close()
    assert r.verdict == "ok" and r.walks == 20000 and r.max_depth > 18, dict(r)


def test_request_stop_ends_an_unbounded_simulation(amd):
    eng = amd.Engine("atomic_add", [10], **SMALL)
    eng.set_progress(lambda *a: eng.request_stop(), 0.0)
    r = eng.simulate(0, 100, 9)
    eng.close()
    assert r.verdict == "budget" and r.steps > 0


def test_request_stop_ends_an_unbounded_simulation_of_short_walks(amd):
    """walks of at most 5 states end within one launch (6 of its 16 events), so every round of this unbounded run is over after its first
    launch; the progress callback still runs after it, and a stop request ends the run"""
    eng = amd.Engine("atomic_add", [3], **SMALL)
    calls = []

    def stop(*a):
        calls.append(a)
        if len(calls) >= 3:
            eng.request_stop()
    eng.set_progress(stop, 0.0)
    r = eng.simulate(0, 5, 9)
    eng.close()
    walks = 3 * (1 << 18)
    assert (r.verdict, len(calls), r.walks, r.steps, r.max_depth) == ("budget", 3, walks, 5 * walks, 5), dict(r)
    assert [c[3] for c in calls] == [walks // 3, 2 * walks // 3, walks]   # (rounds done, generated, states reached, walks completed)


def test_a_stop_inside_a_round_reports_no_other_walk(amd):
    """the Paxos negative control, walks until its violation; a stop after the first launch either ends the run before the round is
    complete (no violation reported: its lowest-indexed violating walk may not have ended) or after it, with the same walk and trace"""
    params = [0, 3, 2, 2, 15, 0, 3]
    eng = amd.Engine("paxos", params, deadlock=False, **SMALL)
    ref = eng.simulate(0, 100, 5)
    ref_trace = eng.trace()
    eng.set_progress(lambda *a: eng.request_stop(), 0.0)
    r = eng.simulate(0, 100, 5)
    trace = eng.trace() if r.trace_len else None
    eng.close()
    assert ref.verdict == "invariant"
    if r.verdict == "budget":
        assert r.trace_len == 0 and r.violating_walk is None
    else:
        assert (r.verdict, r.violating_walk, r.trace_len) == (ref.verdict, ref.violating_walk, ref.trace_len) and trace == ref_trace


def test_cli_sigint_ends_an_unbounded_simulation():
    """`mc atomic_add.tla -simulate` without num= runs until interrupted: SIGINT prints the report of what was walked, exit status 0"""
    import signal
    import time
    p = subprocess.Popen([str(MC), str(ROOT / "specs" / "atomic_add.tla"), "-simulate", "-seed", "3"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    try:
        time.sleep(4)
        p.send_signal(signal.SIGINT)
        out, err = p.communicate(timeout=60)
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
    assert p.returncode == 0, err
    assert "Simulation stopped; no error has been found so far." in out and "The number of states generated: " in out


def run_mc(*args):
    p = subprocess.run([str(MC), *map(str, args)], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


README_MODEL = ROOT / "specs" / "readme_variant" / "pcal_intro.tla"


def test_cli_simulate_violation_report():
    rc, out, err = run_mc(README_MODEL, "-simulate", "num=100000", "-seed", "1")
    assert rc == 12, err
    assert "Running Random Simulation with seed 1" in out
    assert "The first argument of Assert evaluated to FALSE" in out and "Error: The behavior up to this point is:" in out
    assert "State 1: <Initial predicate>" in out and "The number of states generated: " in out
    assert "distinct states found" not in out and "depth of the complete state graph search" not in out
    rc2, out2, _ = run_mc(README_MODEL, "-simulate", "num=100000", "-seed", "1")
    strip = lambda s: "\n".join(l for l in s.splitlines() if not l.startswith("Finished in"))   # noqa: E731
    assert rc2 == 12 and strip(out2) == strip(out)


def test_cli_simulate_clean_and_deadlock():
    rc, out, err = run_mc(ROOT / "specs" / "atomic_add.tla", "-simulate", "num=500", "-depth", "30", "-seed", "4")
    assert rc == 0, err
    assert "No error has been found." in out and "500 walks" in out and "The number of states generated: " in out
    rc, out, err = run_mc(ROOT / "specs" / "atomic_add.tla", "-simulate", "num=500", "-depth", "30")
    assert rc == 0 and "Running Random Simulation with seed " in out
    voting = ROOT / "specs" / "paxos" / "MCVoting3.tla"   # runs out of ballots: TLC's default deadlock check reports it
    rc, out, err = run_mc(voting, "-unverified", "-simulate", "num=5000", "-seed", "2")
    assert rc == 11, err
    assert "Error: Deadlock reached." in out and "Error: The behavior up to this point is:" in out
    rc, out, err = run_mc(voting, "-unverified", "-deadlock", "-simulate", "num=5000", "-seed", "2")
    assert rc == 0 and "No error has been found." in out, err


@pytest.mark.parametrize("opt", [["-gpus", "2"], ["-dump", "x.txt"], ["-checkpoint", "x.ck"], ["-recover", "x.ck"]])
def test_cli_simulate_refusals(opt):
    rc, out, err = run_mc(README_MODEL, "-simulate", "num=10", *opt)
    assert rc == 1 and f"{opt[0]} is not available with -simulate" in err


def test_cli_simulate_refuses_a_host_evaluated_module(tmp_path):
    (tmp_path / "Tiny.tla").write_text("---- MODULE Tiny ----\nEXTENDS Naturals\nVARIABLE x\nInit == x = 0\nNext == x' = (x + 1) % 3\n"
                                       "Spec == Init /\\ [][Next]_x\n====\n")
    (tmp_path / "Tiny.cfg").write_text("SPECIFICATION Spec\n")
    rc, out, err = run_mc(tmp_path / "Tiny.tla", "-simulate", "num=10")
    assert rc == 1 and "-simulate needs a GPU lowering" in err, (out, err)
