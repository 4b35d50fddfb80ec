"""Simulation mode's walks (tla_rust_amd/csrc/sim_walk.h through tests/_simshim, no GPU) against the ORACLE'S STATE GRAPH: tests/simgraph.py
decides from the graph alone (oracle/bfs.c's edge dump, oracle/tla_eval.py for compiled programs) whether a walk is legal — every step an
in-model, non-stuttering, unflagged edge, the end reason the one the graph gives, nothing walked past a violation, `generated` / `steps` /
`walks` / `max_depth` the sums over the graph — and whether the choices are uniform over the candidates and independent between steps.

What this suite found: the PlusCal families (atomic_add, pcal_intro, compiled programs) do not mark their terminating disjunct
ST_SELFLOOP, so a terminated walk took that stuttering step until `depth`; sim_step now passes over a successor whose row equals its
parent's.  Before the fix `check` failed with "step k stutters" on every such model at depth 16 / 17 / 60.

Mutants of sim_walk.h (test_mutants_are_killed builds each and asserts that `suite` fails) and what kills each:
  stutter-built      a built successor equal to its parent is taken         check: "step k stutters" (pcal_intro)
                     (making only the ST_SELFLOOP successors eligible is an equivalent mutant: the built row equals its parent)
  out-of-model       an ST_OUT_OF_MODEL successor is eligible                check: "leaves the model" (raft)
  depth-off-by-one   wk.t > depth for >=                                     check: "more states than depth"
  deadlock-ignored   the deadlock flag is ignored                            check: end reason of a deadlocked Voting state
  gen-unflagged      `gen` does not count flagged successors                 check: the walk's generated (pcal_intro, Assert)
  init-zero          initial index fixed to 0                                uniformity of the initial state
  step-unhashed      step left out of sim_step_hash                          independence of consecutive choices
  slot-unhashed      slot left out of sim_slot_hash                          uniformity of the successor taken
  parent-unchecked   the reached state's invariant check removed             check: "the graph ends this walk on a violation (1, 2" (paxos:
                                                                             a walk of depth 2 stands in a state that breaks invariant 2)
  violation-passed   the violation is kept but the walk goes on              check: "a violation key on a walk that ended otherwise"
The test asserts that each mutant dies of the failure named here (MUTANTS' third column), not of any failure.
"""
import random
import sys
from collections import Counter
from functools import lru_cache
from pathlib import Path

import pytest

import helpers
import simgraph
import simwalk
import testlib

ROOT = helpers.ROOT
sys.path.insert(0, str(ROOT / "oracle"))

RAFT = [2, 2, 2, 9, 1, 1]   # (its CONSTRAINT bounds the model: out-of-model ends)
MODELS = [
    ("atomic_add", [3], [3]),
    ("atomic_add", [4], [4]),
    ("pcal_intro", [0, 1, 20, 2], [0, 1, 20, 2]),
    ("pcal_intro", [1, 1, 20, 2], [1, 1, 20, 2]),             # MoneyInvariant fails
    ("pcal_intro", [1, 0, 20, 2], [1, 0, 20, 2]),             # the README's Assert fails
    ("raft", RAFT, helpers.raft_oracle_params(RAFT)),
    ("ssi", [2, 2, 127, 0], [2, 2, 127, 0]),
    ("paxos", [1, 3, 2, 2, 1, 0, 1], [1, 3, 2, 2, 1, 0, 1]),  # Voting: deadlocks (no SYMMETRY: the oracle prints other orbit representatives)
    ("paxos", [0, 3, 2, 2, 15, 0, 3], [0, 3, 2, 2, 15, 0, 3]),  # the negative control invariant
]
IDS = [f"{s}{p}" for s, p, _ in MODELS]
DEPTHS = (1, 2, 16, 17, 60)
SEEDS = (1, 2, 3)
N = 300


@lru_cache(maxsize=None)
def graph(spec, oparams):
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        helpers.oracle_graph_files(spec, list(oparams), Path(d) / "states.txt", Path(d) / "edges.txt")
        return simgraph.from_oracle_files(Path(d) / "states.txt", Path(d) / "edges.txt")


def check(tmp, g, spec, params, seed, n, depth, deadlock, L=None, first=0):
    run = simwalk.walks(spec, params, seed=seed, n=n, depth=depth, first=first, deadlock=deadlock, dump=str(tmp / "walks.txt"), L=L)
    texts = simwalk.walk_texts(tmp / "walks.txt", run["walks"])
    return simgraph.check_run(g, run, texts, depth, deadlock, simgraph.INV_ON[spec]), run, texts


def model_ends(tmp, spec, params, oparams, deadlock, L=None, seeds=SEEDS, depths=DEPTHS):
    g, ends = graph(spec, tuple(oparams)), Counter()
    for depth in depths:
        for seed in seeds:
            ends += check(tmp, g, spec, params, seed, N, depth, deadlock, L)[0]
    return ends


@pytest.mark.parametrize("spec,params,oparams", MODELS, ids=IDS)
@pytest.mark.parametrize("deadlock", [True, False])
def test_host_walks_are_walks_of_the_graph(tmp_path, spec, params, oparams, deadlock):
    ends = model_ends(tmp_path, spec, params, oparams, deadlock)
    assert sum(ends.values()) == N * len(DEPTHS) * len(SEEDS) and ends[simgraph.END_DEPTH] >= N * len(SEEDS)


def test_every_end_reason_is_met(tmp_path):
    ends = Counter()
    for spec, params, oparams in MODELS:
        ends += model_ends(tmp_path, spec, params, oparams, False, seeds=(1,), depths=(17, 60))
    ends += model_ends(tmp_path, *MODELS[7], True, seeds=(1,), depths=(60,))
    ends += program_ends(tmp_path, *PROGRAMS[2][:4], depths=(60,))   # the CONSTRAINT-bounded one: out-of-model ends
    assert all(ends[r] > 0 for r in (1, 2, 3, 4, 5)), dict(ends)


def test_walks_of_later_rounds(tmp_path):
    """walks with an index past the engine's first round (2^18) are functions of (seed, index) like any other"""
    g = graph("raft", tuple(helpers.raft_oracle_params(RAFT)))
    check(tmp_path, g, "raft", RAFT, 5, 200, 60, True, first=(1 << 18) - 100)


# ------------------------------------------------------------------------------------------------ compiled PlusCal programs
PROGRAMS = [
    ("cas_counter.tla", ["NeverTooMany", "SeenIsOld"], {"Workers": 2, "N": 2}, [], simgraph.END_STUTTER),
    ("two_phase_soup.tla", ["Consistent", "OneDecision", "PreparedWereSent", "KnownMessages"], {"RM": 3, "Hasty": True}, [], simgraph.END_VIOLATION),
    ("growing_counters.tla", ["NeverAhead"], {"Bound": 6}, ["Small"], simgraph.END_OUT_OF_MODEL),   # an infinite algorithm under a CONSTRAINT
]


def program_ends(tmp, name, invs, consts, constraints, depths=DEPTHS):
    from tla_eval import Checker
    text = (ROOT / "specs" / "pluscal" / name).read_text()
    host = helpers.ShimProgram(text, invariants=invs, constants=consts, constraints=constraints)
    try:
        g = simgraph.from_checker(Checker(host.translated(), constants=consts), invariants=invs, constraints=constraints)
        ends = Counter()
        for depth in depths:
            for deadlock in (True, False):
                ends += check(tmp, g, "pcal", host.params, 11, N, depth, deadlock)[0]
        return ends
    finally:
        host.close()


@pytest.mark.parametrize("name,invs,consts,constraints,reason", PROGRAMS, ids=[p[0] for p in PROGRAMS])
def test_compiled_program_walks_are_walks_of_the_evaluators_graph(tmp_path, name, invs, consts, constraints, reason):
    ends = program_ends(tmp_path, name, invs, consts, constraints)
    assert ends[reason] > 0 and ends[simgraph.END_DEPTH] > 0, dict(ends)


# ------------------------------------------------------------------------------------------------ the reference is not vacuous
def test_tampered_walks_are_rejected(tmp_path):
    spec, params = "pcal_intro", [0, 1, 20, 2]
    g = graph(spec, tuple(params))
    _, run, texts = check(tmp_path, g, spec, params, 4, 50, 60, True)
    k = next(i for i, w in enumerate(run["walks"]) if w["end"] == simgraph.END_STUTTER and w["len"] >= 4)
    tx, end = texts[k][0], run["walks"][k]["end"]

    def ok(t, e, depth=60, deadlock=True, viol=None, gr=g, inv_on="successor"):
        return simgraph.check_walk(gr, t, e, depth, deadlock, inv_on, viol=viol)
    assert ok(tx, end) == run["walks"][k]["gen"]
    other = next(t for t, _ in texts if t[0] != tx[0] and t[-1] != tx[-1])
    tampered = {
        "a non-edge": (tx[:2] + [other[-1]] + tx[3:], end, {}),
        "a stuttering step": (tx[:2] + [tx[1]] + tx[2:], end, {}),
        "a stuttering step at the end": (tx + [tx[-1]], end, {}),
        "not an initial state": (tx[1:], end, {}),
        "a wrong end reason": (tx, simgraph.END_OUT_OF_MODEL, {}),
        "ended early": (tx[:-1], end, {}),
        "depth + 1 states": (tx[:3], simgraph.END_DEPTH, dict(depth=2)),
        "depth reached, other reason": (tx[:2], simgraph.END_DEADLOCK, dict(depth=2)),
        "a violation key on a clean walk": (tx, end, dict(viol=(simgraph.VK_ASSERT, 0, 0))),
    }
    for what, (t, e, kw) in tampered.items():
        with pytest.raises(simgraph.WalkError):
            ok(t, e, **kw)
            pytest.fail(f"accepted: {what}")
    # a walk continued past a violating state, and a violation of the wrong kind (the README model: the Assert at label C)
    spec, params = "pcal_intro", [1, 0, 20, 2]
    g2 = graph(spec, tuple(params))
    _, run, texts = check(tmp_path, g2, spec, params, 4, 2000, 60, True)
    k = next(i for i, w in enumerate(run["walks"]) if w["end"] == simgraph.END_VIOLATION)
    tx, viol = texts[k][0], simgraph.key_fields(run["walks"][k]["viol"])
    assert viol[0] == simgraph.VK_ASSERT
    ok(tx, 2, viol=viol, gr=g2)
    nxt = next(iter(g2.candidates(tx[-1])), None)
    assert nxt is not None   # (the other process can still move: the walk could have been continued)
    for what, (t, e, v) in {"continued past the violation": (tx + [nxt], 1, None), "kind": (tx, 2, (simgraph.VK_INVARIANT, 0, 0)),
                            "no violation": (tx, simgraph.END_STUTTER, None)}.items():
        with pytest.raises(simgraph.WalkError):
            ok(t, e, depth=len(t), viol=v, gr=g2)
            pytest.fail(f"accepted: {what}")
    # a step into an out-of-model state (raft's CONSTRAINT)
    g3 = graph("raft", tuple(helpers.raft_oracle_params(RAFT)))
    s, e = next((s, e) for s, es in g3.succ.items() for e in es if not e.inmodel and not g3.bad_successors(s, "successor"))
    _, run, texts = check(tmp_path, g3, "raft", RAFT, 4, 300, 60, True)
    tx = next(t for t, _ in texts if s in t)
    with pytest.raises(simgraph.WalkError, match="leaves the model"):
        ok(tx[:tx.index(s) + 1] + [e.text], simgraph.END_DEPTH, depth=tx.index(s) + 2, gr=g3)


# ------------------------------------------------------------------------------------------------ uniformity
# Chi-square tests with fixed seeds (deterministic).  Significance 1e-6 over all of them; the critical value comes from the
# distribution (simgraph.chi2_critical), expected counts per cell are at least 5 (simgraph.chi2_stat asserts it).
TESTS = 4
ALPHA = 1e-6 / TESTS


def accept(observed, weights):
    stat, df = simgraph.chi2_stat(observed, weights)
    return stat <= simgraph.chi2_critical(df, ALPHA), stat, df


def initial_cells(tmp, L=None):
    """pcal_intro with MaxMoney 20: 400 initial states; 40 000 walks of one state"""
    spec, params = "pcal_intro", [0, 1, 20, 2]
    g = graph(spec, tuple(params))
    _, _, texts = check(tmp, g, spec, params, 8, 40000, 1, True, L)
    return Counter(t[0] for t, _ in texts), Counter(e.text for e in g.init if e.inmodel)


def successor_cells(tmp, L=None):
    """the successor taken from the most-visited states of two models: atomic_add's initial state, raft's initial state"""
    out = []
    for spec, params, oparams, n in (("atomic_add", [4], [4], 4000), ("raft", RAFT, helpers.raft_oracle_params(RAFT), 4000)):
        g = graph(spec, tuple(oparams))
        _, _, texts = check(tmp, g, spec, params, 9, n, 2, True, L)
        s0 = texts[0][0][0]
        assert all(t[0] == s0 for t, _ in texts)
        out.append((Counter(t[1] for t, _ in texts), g.candidates(s0)))
    return out


def pair_cells(tmp, L=None):
    """independence of consecutive choices.  Not on atomic_add, the model the issue names: there a slot is spent once taken, so a chooser
    that forgets the step walks a random permutation of the adders, which has exactly the distribution of independent uniform choices
    among the adders left (nothing to detect).  The README pcal_intro instead, where both processes stay enabled over the first steps, so every one of
    the first two states of a walk has two candidates.  Cell = (rank of choice 1, rank of choice 2) among the sorted candidates; a
    chooser that forgets the step orders the slots alike at both steps."""
    spec, params = "pcal_intro", [1, 1, 20, 2]
    g = graph(spec, tuple(params))
    _, _, texts = check(tmp, g, spec, params, 10, 8000, 3, True, L)
    cells = Counter()
    for t, _ in texts:
        c1, c2 = sorted(g.candidates(t[0])), sorted(g.candidates(t[1]))
        if len(t) == 3 and len(c1) == 2 and len(c2) == 2:
            cells[(c1.index(t[1]), c2.index(t[2]))] += 1
    assert sum(cells.values()) > 2000
    return cells, {(a, b): 1 for a in (0, 1) for b in (0, 1)}


def uniformity(tmp, L=None):
    """the four chi-square tests made on a walk library; AssertionError names the first that fails.  Successor weights are the oracle's
    edge multiplicities: they agree with the enabled slots per edge on both models (per-walk `generated` is compared exactly)"""
    ok, stat, df = accept(*initial_cells(tmp, L))
    assert ok, f"not uniform: the initial state ({stat:.1f}, {df} degrees of freedom)"
    made = 1
    for (o, w), model in zip(successor_cells(tmp, L), ("atomic_add", "raft")):
        ok, stat, df = accept(o, w)
        assert ok, f"not uniform: the successor taken, {model} ({stat:.1f}, {df} degrees of freedom)"
        made += 1
    ok, stat, df = accept(*pair_cells(tmp, L))
    assert ok, f"not independent: consecutive choices ({stat:.1f}, {df} degrees of freedom)"
    assert made + 1 == TESTS


def test_choices_are_uniform_and_independent(tmp_path):
    uniformity(tmp_path)


def test_uniformity_controls(tmp_path):
    """a reference sampler with the same sizes and weights passes; samplers that favour some cells by three tenths fail"""
    rng = random.Random(2024)
    _, w = initial_cells(tmp_path)
    cells = list(w)
    assert accept(Counter(rng.choices(cells, [w[c] for c in cells], k=40000)), w)[0]
    assert not accept(Counter(rng.choices(cells, [w[c] * (1.3 if k % 2 else 1) for k, c in enumerate(cells)], k=40000)), w)[0]
    four = {k: 1 for k in range(4)}
    assert accept(Counter(rng.choices(range(4), k=4000)), four)[0]
    assert not accept(Counter(rng.choices(range(4), [1.3, 1, 1, 1], k=4000)), four)[0]
    assert abs(simgraph.chi2_sf(simgraph.chi2_critical(399, ALPHA), 399) - ALPHA) < ALPHA * 1e-6
    assert abs(simgraph.chi2_sf(3.841458820694124, 1) - 0.05) < 1e-12 and abs(simgraph.chi2_sf(18.307038053275146, 10) - 0.05) < 1e-12


# ------------------------------------------------------------------------------------------------ mutants
# name: (text of sim_walk.h, its replacement, what the failure that kills the mutant must say)
MUTANTS = {
    "stutter-built": ("if (same) {", "if (false && same) {", "stutters"),
    "out-of-model": ("else if (!(st & ST_OUT_OF_MODEL)) {", "else {", "leaves the model"),
    "depth-off-by-one": ("} else if (wk.t >= depth) {", "} else if (wk.t > depth) {", "more states than depth"),
    "deadlock-ignored": ("if (deadlock) { wk.viol =", "if (false) { wk.viol =", "the graph ends this walk on a violation [(3, 0"),
    "gen-unflagged": ("if (first) ++gen;", "if (first && !(st & (ST_ASSERT | ST_SPECERR | ST_INVARIANT))) ++gen;", "the walk's generated is"),
    "init-zero": ("S::init(prm, ni ? wk.hash % ni : 0, nxt);", "S::init(prm, 0, nxt);", "not uniform: the initial state"),
    "step-unhashed": ("return fmix64(walk_hash ^ ((uint64_t)step * 0xc2b2ae3d27d4eb4full));", "return fmix64(walk_hash);", "not independent"),
    "slot-unhashed": ("((uint64_t)slot + 1u) * 0x165667b19e3779f9ull", "1u * 0x165667b19e3779f9ull", "not uniform: the successor taken"),
    "parent-unchecked": ("if (ps & ST_INVARIANT) {", "if (false) {", "the graph ends this walk on a violation [(1, 2"),
    "violation-passed": ("if (viol != ~0ull) { wk.viol = viol; wk.end = SIM_END_VIOLATION; continue; }", "if (viol != ~0ull) { wk.viol = viol; }",
                         "a violation key on a walk that ended otherwise"),
}


def suite(tmp, L=None):
    """what the tests above assert, short: raises AssertionError (simgraph.WalkError is one) when a walk library fails any of it"""
    for k in (1, 3, 4, 5, 7, 8):
        spec, params, oparams = MODELS[k]
        for deadlock in (True, False):
            model_ends(tmp, spec, params, oparams, deadlock, L, seeds=(1,), depths=(2, 17, 60))
    uniformity(tmp, L)


def test_the_product_passes_the_short_suite(tmp_path):
    suite(tmp_path)


def test_mutants_are_killed(tmp_path):
    helpers.build_shim()

    def build(name):
        return simwalk.build_simshim(csrc=testlib.mutant_tree(tmp_path, name, ("sim_walk.h", *MUTANTS[name][:2])), out=tmp_path / name / "_build")
    killed_by = {}
    for name, so in testlib.build_mutants(MUTANTS, build).items():
        with pytest.raises(AssertionError) as e:
            suite(tmp_path, simwalk.load(so))
            pytest.fail(f"mutant {name} survives", pytrace=False)
        killed_by[name] = str(e.value)
        assert MUTANTS[name][2] in killed_by[name], (name, killed_by[name][:300])
    print({k: v[:80] for k, v in killed_by.items()})


def raft_slice(args):
    """(generated, steps, walks, max_depth) of host walks first .. first + n - 1 of the raft model, each judged by the graph reference
    and the slice's counters summed from the graph (simgraph.check_run).  A function of its own so that
    tests/test_gpu_simulate_graph.py can spread a million walks over processes."""
    import tempfile
    seed, first, n, depth = args
    g = graph("raft", tuple(helpers.raft_oracle_params(RAFT)))
    with tempfile.TemporaryDirectory() as d:
        _, run, _ = check(Path(d), g, "raft", RAFT, seed, n, depth, True, first=first)
    return run["generated"], run["steps"], run["walks_done"], run["max_depth"]
