"""-coverage on the device (MC_F_COVERAGE: k_coverage_generated / k_coverage_distinct of engine_coverage.h, mc_engine_coverage, `mc X.tla
-coverage`) against the oracle's state graph, action name by action name: generated[a] = the oracle's edges of action a out of the
levels the search expanded, distinct[a] between the bounds the graph gives for "first to find" (tests/covshim.py OracleGraph), the sums
= mc_result's; at every budget, on a violating model, with the flag changing nothing else, on compiled programs (interpreter = generated
code = oracle/tla_eval.py label by label), across mc_engine_step, and in mc's report."""
import subprocess
import sys
from collections import Counter
from functools import lru_cache
from pathlib import Path

import pytest

import covshim
import helpers

ROOT = Path(__file__).resolve().parent.parent
S = ROOT / "specs"
sys.path.insert(0, str(ROOT / "oracle"))
pytestmark = pytest.mark.gpu
KW = dict(table_capacity=1 << 20, arena_capacity=1 << 18, chunk_states=1 << 12)   # (several chunks per level on the larger models)
RAFT = [2, 2, 2, 9, 1, 1]


@pytest.fixture(scope="module")
def amd():
    import tla_rust_amd
    assert tla_rust_amd.device_count() >= 1, "no HIP device visible"
    return tla_rust_amd


def raft_small(amd):
    r = amd.ResolvedSpec(S / "MCraft.tla", S / "MCraft_small.cfg", unverified=True)
    assert r.spec == "raft"
    return list(r.params)


# (spec, engine params or a function of amd that gives them, deadlock checking)
MODELS = {
    "atomic_add3": ("atomic_add", [3], True),
    "pcal_intro": ("pcal_intro", [0, 1, 20, 2], True),
    "pcal_intro_readme": ("pcal_intro", [1, 0, 20, 2], True),     # the README's variant: the Assert at C fails
    "pcal_intro_invariant": ("pcal_intro", [1, 1, 20, 2], True),  # ... with MoneyInvariant checked: violated
    "raft2": ("raft", RAFT, True),
    "ssi2x2": ("ssi", [2, 2, 127, 0], True),
    "voting": ("paxos", [1, 3, 2, 2, 1, 0, 1], False),
    "raft_small_cfg": ("raft", raft_small, True),
}
CLEAN = ["atomic_add3", "pcal_intro", "raft2", "ssi2x2", "voting", "raft_small_cfg"]


def model(amd, key):
    spec, params, deadlock = MODELS[key]
    params = params(amd) if callable(params) else params
    return spec, params, (helpers.raft_oracle_params(params) if spec == "raft" else params), deadlock


_graphs = {}


def graph(tmp_path_factory, spec, oparams, deadlock):
    k = (spec, tuple(oparams), deadlock)
    if k not in _graphs:
        _graphs[k] = covshim.OracleGraph(spec, oparams, tmp_path_factory.mktemp("graph"), check_deadlock=deadlock)
    return _graphs[k]


def check_against_graph(g, cov, r, expanded):
    """cov: Engine.coverage() of a search that expanded levels 1 .. expanded (None: all) and returned r"""
    want = g.generated(expanded)
    lower, upper, stored = g.distinct_bounds(expanded)
    print("levels", expanded, "coverage", cov, "oracle generated", dict(want), "bounds", dict(lower), dict(upper))
    assert set(want) <= set(cov), set(want) - set(cov)
    for name, (d, n) in cov.items():
        assert n == want[name], f"generated[{name}] = {n}: the oracle's graph has {want[name]} such edges out of the expanded levels"
        assert lower[name] <= d <= upper[name], f"distinct[{name}] = {d} outside [{lower[name]}, {upper[name]}]"
        assert n > 0 or d == 0
    init_edges = [e for e in g.edges if e[0] < 0]
    assert cov["Init"] == (sum(1 for lv in g.level if lv == 1), len(init_edges))
    assert sum(n for _, n in cov.values()) == r.generated and sum(d for d, _ in cov.values()) == r.distinct == stored


@pytest.mark.parametrize("key", CLEAN)
def test_counts_are_the_oracles_per_action_at_every_budget(amd, tmp_path_factory, key):
    spec, params, oparams, deadlock = model(amd, key)
    g = graph(tmp_path_factory, spec, oparams, deadlock)
    budgets = [0, 3, max(4, g.depth - 1)]   # unlimited; two budgets: early, and all but the last level
    for ml in budgets:
        eng = amd.Engine(spec, params, deadlock=deadlock, coverage=True, max_levels=ml, **KW)
        r = eng.run()
        cov = eng.coverage()
        eng.close()
        if ml:
            assert r.verdict == "budget" and len(r.levels) == ml, (ml, r.verdict, len(r.levels))
        else:
            assert r.verdict in ("ok", "deadlock") and len(r.levels) == g.depth
        # max_levels = M: levels 1 .. M - 1 were expanded, level M was found and is the queue
        check_against_graph(g, cov, r, ml - 1 if ml else None)


@pytest.mark.parametrize("key", ["pcal_intro_readme", "pcal_intro_invariant"])
def test_counts_stop_at_the_end_of_the_violating_level(amd, tmp_path_factory, key):
    spec, params, oparams, deadlock = model(amd, key)
    g = graph(tmp_path_factory, spec, oparams, deadlock)
    o = helpers.oracle_run(spec, oparams, stop=1)   # stops at the end of the level that found the violation
    assert o["verdict"] in ("assert", "invariant")
    # the levels that run expanded, from the oracle's own counts: the E whose edges (+ Init) are its `generated`
    expanded = [e for e in range(1, g.depth + 1) if sum(g.generated(e).values()) == o["generated"]]
    assert len(expanded) >= 1
    eng = amd.Engine(spec, params, coverage=True, **KW)
    r = eng.run()
    cov = eng.coverage()
    eng.close()
    assert (r.verdict, r.generated, r.distinct) == (o["verdict"], o["generated"], o["distinct"])
    check_against_graph(g, cov, r, expanded[0])


def check_trace_is_a_path(g, trace, verdict):
    """trace: Engine.trace() of a run that ended on an Assert: [(action name, state text)]"""
    texts = [s.replace("\n", " ") for _, s in trace]
    assert trace[0][0] == "Initial predicate" and g.level[g.index[texts[0]]] == 1
    out = {}
    for par, name, flags, _inmodel, text in g.edges:
        if par >= 0:
            out.setdefault(par, []).append((name, flags, text))
    for k in range(1, len(trace)):
        assert (trace[k][0], texts[k]) in {(n, t) for n, f, t in out[g.index[texts[k - 1]]] if not f & 3}, (k, trace[k])
    assert verdict == "assert" and any(f & 1 for _, f, _ in out[g.index[texts[-1]]]), "the last state has no successor that fails its Assert"


@pytest.mark.parametrize("key", ["raft2", "ssi2x2", "pcal_intro_readme", "atomic_add3"])
@pytest.mark.parametrize("debug_flags", [0, 32])
def test_the_flag_changes_nothing_else(amd, tmp_path_factory, key, debug_flags):
    spec, params, oparams, deadlock = model(amd, key)
    a = amd.Engine(spec, params, deadlock=deadlock, debug_flags=debug_flags, **KW)
    b = amd.Engine(spec, params, deadlock=deadlock, debug_flags=debug_flags, coverage=True, **KW)
    ra, rb = a.run(), b.run()
    for k in ("distinct", "generated", "depth", "levels", "verdict", "queue_left", "violated_invariant", "trace_len"):
        assert ra[k] == rb[k], (k, ra[k], rb[k])
    # Which of a level's violations is reported follows the arena order, which is the engine's race (two runs without the flag differ
    # too): what holds for every run is the length, and that the behaviour is a path of the oracle's graph from an initial state to a
    # state with a successor of the reported kind
    ta, tb = a.trace(), b.trace()
    assert len(ta) == len(tb) == (ra.trace_len if ra.verdict != "ok" else 0)
    if ta:
        g = graph(tmp_path_factory, spec, oparams, deadlock)
        for tr in (ta, tb):
            check_trace_is_a_path(g, tr, ra.verdict)
    cov = b.coverage()
    assert sum(n for _, n in cov.values()) == rb.generated and sum(d for d, _ in cov.values()) == rb.distinct
    with pytest.raises(amd.McError) as e:
        a.coverage()
    assert e.value.code == -7   # MC_ESTATE
    a.close()
    b.close()


def test_traced_off_engine_still_counts(amd):
    """MC_F_COVERAGE implies MC_F_TRACE"""
    eng = amd.Engine("atomic_add", [3], trace=False, coverage=True, **KW)
    r = eng.run()
    cov = eng.coverage()
    eng.close()
    assert sum(d for d, _ in cov.values()) == r.distinct == 9 and cov["Increment"] == (7, 12)


def test_step_accumulates_and_a_new_search_starts_over(amd):
    spec, params = "raft", RAFT
    whole = amd.Engine(spec, params, coverage=True, **KW)
    rw = whole.run()
    cw = whole.coverage()
    eng = amd.Engine(spec, params, coverage=True, **KW)
    r1 = eng.step(2)
    c1 = eng.coverage()
    assert r1.verdict == "budget" and sum(n for _, n in c1.values()) == r1.generated and sum(d for d, _ in c1.values()) == r1.distinct
    r2 = eng.step(4096 - 8)
    c2 = eng.coverage()
    assert (r2.verdict, r2.distinct, r2.generated) == (rw.verdict, rw.distinct, rw.generated)
    assert {k: v[1] for k, v in c2.items()} == {k: v[1] for k, v in cw.items()}
    assert sum(d for d, _ in c2.values()) == rw.distinct
    r3 = eng.step(2)   # the search had ended: this one starts over, and so do its counts
    assert {k: v[1] for k, v in eng.coverage().items()} == {k: v[1] for k, v in c1.items()} and r3.generated == r1.generated
    r4 = whole.run()   # ... and so does a second run
    assert {k: v[1] for k, v in whole.coverage().items()} == {k: v[1] for k, v in cw.items()} and r4.generated == rw.generated
    eng.close()
    whole.close()


def test_a_restored_run_recounts_the_checkpointed_levels(amd, tmp_path):
    """mc refuses -coverage -recover; an engine that continues a checkpoint counts the levels the file holds from its arena and parent pointers"""
    whole = amd.Engine("raft", RAFT, coverage=True, **KW)
    rw = whole.run()
    cw = whole.coverage()
    whole.close()
    a = amd.Engine("raft", RAFT, max_levels=7, **KW)   # (written without the flag: the trace records are what the recount needs)
    assert a.run().verdict == "budget"
    a.checkpoint(tmp_path / "raft.ck")
    a.close()
    b = amd.Engine("raft", RAFT, coverage=True, **KW)
    b.restore(tmp_path / "raft.ck")
    rb = b.run()
    cb = b.coverage()
    b.close()
    assert (rb.verdict, rb.distinct, rb.generated) == (rw.verdict, rw.distinct, rw.generated)
    assert {k: v[1] for k, v in cb.items()} == {k: v[1] for k, v in cw.items()}
    assert sum(d for d, _ in cb.values()) == rb.distinct and cb["Init"] == cw["Init"]


def test_a_sharded_engine_refuses_the_flag(amd):
    with pytest.raises(amd.McError) as e:
        amd.Engine("atomic_add", [3], coverage=True, shard_rank=0, shard_count=2, **KW)
    assert e.value.code == -1 and "sharded" in str(e.value)


# ------------------------------------------------------------------------------------------------ compiled programs
def program(amd, stem, consts=None, invs=None):
    from test_gpu_pcal import cfg_text
    from test_pcal import CASES
    path, cinvs, cconsts = next(c for c in CASES if c[0].stem == stem and (consts is None or c[2] == consts))
    return amd.Program(path.read_text(), cfg_text(cinvs if invs is None else invs, cconsts)), path, cconsts


@pytest.mark.parametrize("path,spec,params", [(S / "pcal_intro.tla", "pcal_intro", [0, 1, 20, 2]), (S / "atomic_add.tla", "atomic_add", None)])
def test_the_generic_path_gives_the_hand_lowerings_rows(amd, path, spec, params):
    hand = amd.ResolvedSpec(path)
    gen = amd.ResolvedSpec(path, generic=True)
    assert hand.spec == spec and gen.spec == "pcal" and (params is None or list(hand.params) == params)
    a = amd.Engine(hand.spec, hand.params, coverage=True, **KW)
    b = amd.Engine(gen.spec, gen.params, coverage=True, **KW)
    ra, rb = a.run(), b.run()
    ca, cb = a.coverage(), b.coverage()
    a.close()
    b.close()
    assert (ra.distinct, ra.generated) == (rb.distinct, rb.generated)
    # label by label; a row the hand lowering lists for a label this variant of the algorithm does not have is 0 : 0 there
    assert {k: v[1] for k, v in cb.items()} == {k: v[1] for k, v in ca.items() if k in cb}, (ca, cb)
    assert all(v == (0, 0) for k, v in ca.items() if k not in cb)
    gen.close()
    hand.close()


@pytest.mark.parametrize("stem", ["peterson", "treiber_stack", "two_phase_channels", "two_phase_soup"])
def test_interpreter_and_generated_code_agree_per_label(amd, stem):
    prog, _, _ = program(amd, stem)
    a = amd.Engine("pcal", prog.params, coverage=True, **KW)
    b = amd.Engine("pcal", prog.params, coverage=True, jit=True, **KW)   # (the soup: sets of records, interpreted either way)
    ra, rb = a.run(), b.run()
    ca, cb = a.coverage(), b.coverage()
    a.close()
    b.close()
    prog.close()
    assert (ra.distinct, ra.generated, ra.verdict) == (rb.distinct, rb.generated, rb.verdict)
    assert list(ca) == list(cb) and "Done" not in ca and list(ca)[0] == "Init" and list(ca)[-1] == "Terminating"
    assert {k: v[1] for k, v in ca.items()} == {k: v[1] for k, v in cb.items()}
    for c, r in ((ca, ra), (cb, rb)):
        assert sum(n for _, n in c.values()) == r.generated and sum(d for d, _ in c.values()) == r.distinct


@pytest.mark.parametrize("stem", ["peterson", "ticket_lock"])
def test_generated_per_label_equals_the_tla_evaluator(amd, stem):
    """oracle/tla_eval.py on the translation: every label's defined action, per process, over every state of the graph"""
    from tla_eval import Checker
    prog, _, consts = program(amd, stem)
    eng = amd.Engine("pcal", prog.params, coverage=True, **KW)
    r = eng.run()
    cov = eng.coverage()
    eng.close()
    ck = Checker(prog.translated(), constants=consts)
    prog.close()
    o = ck.run_levels(invariants=[])
    assert r.verdict == "ok" and (r.distinct, r.generated) == (o["distinct"], o["generated"])
    ck.engine_mode = True
    seen, todo, states = set(), [], []
    for s in ck.initial_states():
        if ck.key(s) not in seen:
            seen.add(ck.key(s))
            todo.append(s)
    while todo:
        s = todo.pop()
        states.append(s)
        for n in ck.successors(s):
            if "__assert__" not in n and ck.key(n) not in seen:
                seen.add(ck.key(n))
                todo.append(n)
    assert len(states) == o["distinct"]
    def disjuncts(e):
        if e[0] == "disj" or (e[0] == "op" and e[1] == "\\/"):
            for x in (e[1] if e[0] == "disj" else [e[2], e[3]]):
                yield from disjuncts(x)
        else:
            yield e
    # the disjunct of Next that is no process's: (\A self \in ProcSet: pc[self] = "Done") /\ UNCHANGED vars (an algorithm that never ends has none)
    ending = [d for d in disjuncts(ck.defs["Next"][1]) if "unchanged" in repr(d) and "'Done'" in repr(d)]
    assert len(ending) <= 1
    want = Counter()
    for s in states:
        want["Terminating"] += sum(1 for d in ending for _ in ck.act(d, s, {}, {}))
        procs = sorted(ck.ev(ck.defs["ProcSet"][1], s, None, {}), key=repr)
        for name in cov:
            if name in ("Init", "Terminating"):
                continue
            params, body = ck.defs[name]
            for bd in ([{"self": p} for p in procs] if params else [{}]):
                want[name] += sum(1 for _ in ck.act(body, s, {}, bd))
    ck.engine_mode = False
    want["Init"] = sum(1 for _ in ck.initial_states())
    print(stem, "coverage", cov, "evaluator", dict(want))
    assert {k: v[1] for k, v in cov.items()} == {k: want[k] for k in cov}
    assert sum(want.values()) == o["generated"]


# ------------------------------------------------------------------------------------------------ mc
def run_mc(*args):
    import tla_rust_amd.build as b
    b.build()
    return subprocess.run([str(ROOT / "tla_rust_amd" / "_build" / "mc"), *map(str, args), "-noprogress"], capture_output=True, text=True, timeout=600)


def coverage_block(out):
    lines = out.splitlines()
    a, b = lines.index("The coverage statistics :"), lines.index("End of statistics.")
    rows = {}
    for ln in lines[a + 1:b]:
        name, counts = ln.rsplit(": ", 1)
        assert name[0] == "<" and name[-1] == ">"
        d, n = counts.split(":")
        rows[name[1:-1]] = (int(d), int(n))
    return rows, lines[:a] + lines[b + 1:], lines[b + 1]


def test_mc_coverage_shows_the_dead_label():
    p = run_mc(S / "pluscal" / "dead_label.tla", "-coverage")
    assert p.returncode == 0, (p.stdout, p.stderr)
    rows, rest, after = coverage_block(p.stdout)
    assert list(rows) == ["Init", "Enter", "Work", "Check", "Panic", "Leave", "Terminating"]
    assert rows["Panic"] == (0, 0) and all(d > 0 and n > 0 for k, (d, n) in rows.items() if k not in ("Panic", "Terminating")), rows
    assert rows["Terminating"][1] > 0   # (the terminating disjunct stutters: it generates, and finds nothing)
    assert "states generated" in after and "Model checking completed. No error has been found." in p.stdout
    g, d = (int(after.split()[0]), int(after.split()[3]))
    assert sum(n for _, n in rows.values()) == g and sum(x for x, _ in rows.values()) == d
    # without the option: today's report, which is the report above without the block
    q = run_mc(S / "pluscal" / "dead_label.tla")
    assert q.returncode == 0 and "coverage" not in q.stdout and q.stdout.splitlines() == rest
    # TLC's minutes argument, and the option on a hand lowering under -jit / auto-jit settings that do not apply to it
    p5 = run_mc(S / "pluscal" / "dead_label.tla", "-coverage", "5")
    assert p5.returncode == 0 and coverage_block(p5.stdout)[0] == rows


def test_mc_coverage_on_generated_code_and_a_violating_model():
    p = run_mc(S / "pluscal" / "dead_label.tla", "-coverage", "-jit")
    assert p.returncode == 0, (p.stdout, p.stderr)
    rows, _, _ = coverage_block(p.stdout)
    q = run_mc(S / "pluscal" / "dead_label.tla", "-coverage")
    assert {k: v[1] for k, v in rows.items()} == {k: v[1] for k, v in coverage_block(q.stdout)[0].items()} and rows["Panic"] == (0, 0)
    v = run_mc(S / "readme_variant" / "pcal_intro.tla", "-coverage")
    assert v.returncode == 12, (v.stdout, v.stderr)
    rows, _, after = coverage_block(v.stdout)
    assert list(rows) == ["Init", "Transfer", "A", "B", "C", "Terminating"] and "states generated" in after
    assert sum(n for _, n in rows.values()) == int(after.split()[0])


def test_mc_coverage_on_a_host_evaluated_module(tmp_path):
    (tmp_path / "Tiny.tla").write_text("---- MODULE Tiny ----\nEXTENDS Naturals\nVARIABLE x\nInit == x = 0\nNext == x' = (x + 1) % 3\n====\n")
    (tmp_path / "Tiny.cfg").write_text("INIT Init\nNEXT Next\n")
    p = run_mc(tmp_path / "Tiny.tla", "-coverage")
    assert p.returncode == 0, (p.stdout, p.stderr)
    lines = p.stdout.splitlines()
    w = lines.index("Warning: -coverage is not available for a module evaluated on the host")
    assert w < lines.index("Model checking completed. No error has been found.") and "The coverage statistics :" not in lines
    q = run_mc(tmp_path / "Tiny.tla")
    assert q.stdout.splitlines() == lines[:w] + lines[w + 1:]
