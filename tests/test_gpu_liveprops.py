"""<>Q, []<>Q, <>[]P and P ~> Q of fair PlusCal algorithms on the device (mc_engine_predicates, mc_engine_liveness_check, the
counterexample of mc_engine_liveness_trace, `mc X.tla` with such a PROPERTY), interpreter and generated code, against tests/liveprops.py
— oracle/tla_eval.py over the translation and the rule restated from DESIGN.md section 17 — by state text; the least-index rules of
the engine (witness, the way into the component) are the reference's under the engine's own order of the states."""
import re

import numpy as np
import pytest

import helpers
import livegraph
import liveprops
from test_gpu_coverage import KW, amd, model  # noqa: F401  (amd: the fixture)
from test_gpu_graph import run_mc

pytestmark = pytest.mark.gpu
ROOT = helpers.ROOT
MC_EBADCFG, MC_ENOSPEC, MC_ESTATE = -1, -9, -7
BACKENDS = pytest.mark.parametrize("jit", [False, True], ids=["interpreter", "jit"])

_refs = {}


def reference(name):
    """(program, PropGraph) of a model, built once and left unchanged"""
    if name not in _refs:
        _refs[name] = liveprops.load(name)
    return _refs[name]


class Run:
    """one finished search per (model, back end), shared by the tests: everything they ask of it is rebuilt on demand"""

    def __init__(self, amd, name, jit):  # noqa: F811
        self.prog, self.g = reference(name)
        self.eng = amd.Engine("pcal", self.prog.params, jit=jit, **KW)
        r = self.eng.run()
        assert r.verdict == "ok" and r.queue_left == 0
        self.n = r.distinct
        self.texts = [t.replace("\n", " ") for t in self.eng.state_texts(0, self.n)]
        assert sorted(self.texts) == sorted(self.g.texts)
        self.at = {t: i for i, t in enumerate(self.texts)}          # state text -> arena index
        self.rank = [self.at[t] for t in self.g.texts]               # reference number -> arena index
        self.checks = [lp for lp in self.prog.live_properties if not lp["refused"]]

    def want(self, lp):
        return liveprops.decide_model(self.g, lp, self.prog.fair_mask, rank=self.rank)

    def arena(self, states):
        return sorted(self.rank[v] for v in states)


@pytest.fixture(scope="module")
def runs(amd):  # noqa: F811
    made = {}

    def get(name, jit):
        if (name, jit) not in made:
            made[name, jit] = Run(amd, name, jit)
        return made[name, jit]
    yield get
    for r in made.values():
        r.eng.close()


@BACKENDS
@pytest.mark.parametrize("name", list(liveprops.MODELS))
def test_predicate_bits(runs, name, jit):
    r = runs(name, jit)
    bits = r.eng.predicates(r.n)
    assert len(bits) == r.n and dict(zip(r.texts, bits.tolist())) == dict(zip(r.g.texts, r.g.bits))
    assert np.array_equal(bits, r.eng.predicates())   # (on a graph built anew)


@BACKENDS
@pytest.mark.parametrize("name", list(liveprops.MODELS))
def test_every_check_equals_the_reference(runs, name, jit):
    r = runs(name, jit)
    assert {lp["name"] for lp in r.checks} == set(liveprops.MODELS[name].expect)
    r.eng.scc()   # (components and everything kept with them built anew: the first check of a mask builds that mask's)
    masks = set()
    for lp in r.checks:
        want = r.want(lp)
        ci = r.eng.check_property(r.prog.fair_mask, lp)
        print(name, lp["name"], jit, dict(ci))
        assert ci.violated == (1 if want.violated else 0) == (1 if liveprops.MODELS[name].expect[lp["name"]] else 0)
        assert ci.fair_components == len(want.violating) and ci.mask_states == want.mask_states and ci.bad_starts == want.bad_starts
        key = -1 if lp["kind"] == liveprops.STABLE else lp["q"]
        assert ci.scc_builds == (0 if key in masks or key < 0 else 1)   # one build per distinct mask; <>[]P uses the full graph's
        masks.add(key)
        if want.violated:
            assert r.texts[ci.witness] == r.g.texts[want.witness]                      # the least S state that reaches a violating component
            assert ci.witness == min(r.rank[v] for v in starts_of(r, lp, want))
            assert ci.root == min(r.arena(want.root)) and ci.root_size == len(want.root)
        # the components the check judged: those of the induced subgraph, ids the least arena index, outside M its own
        comp = r.eng.check_components(r.n).tolist()
        mine = {}
        for v, c in enumerate(comp):
            mine.setdefault(c, set()).add(v)
            assert c == min(mine[c])
        ref = {}
        for v, c in enumerate(want.comp):
            ref.setdefault(c, set()).add(r.rank[v])
        assert {frozenset(m) for m in mine.values()} == {frozenset(m) for m in ref.values()}
        again = r.eng.check_property(r.prog.fair_mask, lp)
        assert {k: v for k, v in again.items() if k not in ("seconds", "scc_builds")} == {k: v for k, v in ci.items() if k not in ("seconds", "scc_builds")}
        assert again.scc_builds == 0
    # the full graph's components are untouched by the masked builds
    scc = r.eng.scc_read(0, r.n)
    info, offsets, dst, _ = r.eng.graph()
    off, d = offsets.astype(np.int64).tolist(), dst.tolist()
    assert np.array_equal(scc, np.array(livegraph.tarjan(info.states, lambda v: d[off[v]:off[v + 1]]), dtype=np.uint32))


def starts_of(r, lp, want):
    """the reference's bad starts: the S states of M with a way inside M to a violating component"""
    M, S, _ = liveprops.sets(lp["kind"], lp["p"], lp["q"], r.g.bits, len(r.g.init))
    bad = set().union(*want.violating) if want.violating else set()
    reach, todo = set(bad), list(bad)
    pred = {}
    for v, out in enumerate(r.g.edges):
        for _, j in out:
            if M[v] and M[j]:
                pred.setdefault(j, []).append(v)
    while todo:
        for u in pred.get(todo.pop(), []):
            if u not in reach:
                reach.add(u)
                todo.append(u)
    return [v for v in reach if S[v] and M[v]]


VIOLATED = [(n, k) for n, m in liveprops.MODELS.items() for k, v in m.expect.items() if v]


@BACKENDS
@pytest.mark.parametrize("name,prop", VIOLATED, ids=[f"{n}-{k}" for n, k in VIOLATED])
def test_counterexample(runs, name, prop, jit):
    r = runs(name, jit)
    g = r.g
    lp = next(x for x in r.checks if x["name"] == prop)
    ci = r.eng.check_property(r.prog.fair_mask, lp)
    assert ci.violated == 1
    prefix, cycle = r.eng.liveness_trace()
    assert (prefix, cycle) == r.eng.liveness_trace()                              # deterministic
    assert r.eng.check_property(r.prog.fair_mask, lp).violated == 1 and (prefix, cycle) == r.eng.liveness_trace()   # ... across two checks
    M, S, T = liveprops.sets(lp["kind"], lp["p"], lp["q"], g.bits, len(g.init))
    ref = lambda v: g.index[r.texts[v]]   # noqa: E731  (arena index -> the reference's number)
    info, offsets, dst, _ = r.eng.graph()   # (rebuilds the graph: the trace above was read first)
    off = offsets.astype(np.int64).tolist()
    row = lambda v: dst[off[v]:off[v + 1]].tolist()  # noqa: E731
    assert prefix[0] < info.init_states                                           # starts at an initial state
    for u, v in zip(prefix, prefix[1:]):
        assert v in row(u)                                                        # every step is an edge of graph()
    assert ci.witness in prefix
    w = prefix.index(ci.witness)
    assert S[ref(ci.witness)] and all(M[ref(v)] for v in prefix[w:])              # reaches an S state; from there every state is in M
    want = r.want(lp)
    assert prefix[w:] == [r.rank[v] for v in want.path]                           # ... along falling distance, the least successor each time
    fair = {p for p in range(g.nproc) if r.prog.fair_mask >> p & 1}
    stay = prefix[-1]
    if not cycle:   # stuttering: exactly where every fair process is disabled (and the state is a T state)
        assert not (fair & g.en[ref(stay)]) and T[ref(stay)] and M[ref(stay)] and stay in r.arena(want.root)
        if name == "stutter":
            assert len(prefix) == 2
        return
    assert cycle[0] == stay
    walk = cycle + [cycle[0]]
    for u, v in zip(walk, walk[1:]):
        assert v in row(u) and u != v                                             # closed, along edges
    on = [ref(v) for v in cycle]
    assert all(M[i] for i in on) and any(T[i] for i in on)                        # stays inside M, holds a T state
    assert set(cycle) <= set(r.arena(want.root))                                  # inside the chosen component
    taken = set()
    for a, b in zip(on, on[1:] + on[:1]):
        taken |= {p for p, j in g.edges[a] if p >= 0 and j == b and j != a}
    disabled = set()
    for i in on:
        disabled |= set(range(g.nproc)) - g.en[i]
    assert fair <= (taken | disabled), (fair, taken, disabled)                    # the cycle itself meets the fairness condition
    if name == "stable":
        assert len(cycle) == 2   # both states: the walk passes b = 0


RING = [("ring_cut", "ring_cut", 65, 32), ("ring_cut_1000", "ring_cut_1000", 1000, 500)]


@BACKENDS
@pytest.mark.parametrize("label,cfg,n,half", RING, ids=[x[0] for x in RING])
def test_the_cut_ring(amd, label, cfg, n, half, jit):  # noqa: F811
    """one past a wavefront, and four workgroups: the components of the two arcs are Tarjan's on the induced subgraph, the witness is
    c = 1 and the way from it into the final state is half + 1 states long"""
    prog = liveprops.compiled("ring_cut", cfg)
    eng = amd.Engine("pcal", prog.params, jit=jit, **KW)
    try:
        r = eng.run()
        assert r.verdict == "ok" and r.queue_left == 0 and r.distinct == n + 2
        (lp,) = prog.live_properties
        ci = eng.check_property(prog.fair_mask, lp)
        print(label, "jit" if jit else "interpreter", dict(ci), "sweeps", ci.sweeps, "seconds", ci.seconds)
        bits = eng.predicates(r.distinct)
        comp = eng.check_components(r.distinct)
        texts = eng.state_texts(0, r.distinct)
        in_m = [not b & 1 for b in bits.tolist()]
        assert [("c = 0\n" in t or f"c = {half}\n" in t) for t in texts] == [not m for m in in_m]
        assert ci.violated == 1 and ci.mask_states == n and ci.fair_components == 1 and ci.root_size == 1 and ci.scc_builds == 1
        assert ci.witness == 1 and "c = 1\n" in texts[1] and ci.bad_starts == half - 1 + 2
        assert 8 <= ci.sweeps <= n + 2 + 16   # (in place: how far one sweep carries a distance is the scheduler's; the guard's bound is not)
        again = eng.check_property(prog.fair_mask, lp)   # the mask's components are kept: reduction, verdict, reach and witness alone
        print(label, "again", "sweeps", again.sweeps, "seconds", again.seconds)
        assert again.scc_builds == 0 and {k: again[k] for k in again if k not in ("seconds", "scc_builds")} == {k: ci[k] for k in ci if k not in ("seconds", "scc_builds")}
        prefix, cycle = eng.liveness_trace()
        assert cycle == [] and len(prefix) == 1 + half + 1 and prefix[-1] == ci.root and f"c = {half - 1}\n" in texts[ci.root]
        info, offsets, dst, _ = eng.graph()
        off, d = offsets.astype(np.int64).tolist(), dst.tolist()
        want = livegraph.tarjan(info.states, lambda v: [j for j in d[off[v]:off[v + 1]] if in_m[v] and in_m[j]])
        assert comp.tolist() == want and len(set(want)) == n + 2   # (two chains and the stopped states: every state its own component)
    finally:
        eng.close()
        prog.close()


def test_mc_reports_properties(amd):  # noqa: F811
    D = liveprops.DIR
    p = run_mc(D / "stable.tla")
    assert p.returncode == 13, (p.returncode, p.stdout, p.stderr)
    out = p.stdout
    assert "Error: Temporal properties were violated." in out and "Error: The following behavior constitutes a counter-example:" in out
    assert "No error has been found" not in out and "NOT checked" not in out
    numbers = [int(k) for k in re.findall(r"^State (\d+):", out, flags=re.M)]
    assert numbers == list(range(1, len(numbers) + 1)) and numbers
    back = re.findall(r"^Back to state (\d+): <(\w+)>$", out, flags=re.M)
    assert len(back) == 1 and 1 <= int(back[0][0]) <= len(numbers) and back[0][1] == "F"
    p = run_mc(D / "stutter.tla")
    assert p.returncode == 13 and re.search(r"^State 3: Stuttering$", p.stdout, flags=re.M)
    p = run_mc(D / "lost.tla")   # Once holds, Again is violated: the first violated one is reported
    assert p.returncode == 13 and re.search(r"^State 3: Stuttering$", p.stdout, flags=re.M)
    for stem in ("leave_enabled", "mask_split", "peterson_loop", "stable_transient"):
        p = run_mc(D / (stem + ".tla"))
        assert p.returncode == 0 and "No error has been found" in p.stdout, (stem, p.stdout, p.stderr)
        for new in ("Temporal", "temporal", "NOT checked", "Back to state", "Stuttering", "counter-example", "Checking"):
            assert new not in p.stdout, (stem, new)
    p = run_mc(D / "peterson_loop.tla", "-coverage")
    assert p.returncode == 0 and p.stdout.count("Checking temporal property Starvation\n") == 1
    p = run_mc(D / "reach_mask.tla")
    assert p.returncode == 13 and "Back to state" in p.stdout
    for stem, (name, word) in liveprops.REFUSED.items():
        p = run_mc(D / (stem + ".tla"))
        assert p.returncode == 0, (stem, p.stdout, p.stderr)
        warn = [ln for ln in p.stdout.splitlines() if "NOT checked" in ln]
        assert len(warn) == 1 and warn[0].startswith(f"Warning: temporal property {name} NOT checked:") and word in warn[0]
        assert p.stdout.index("NOT checked") < p.stdout.index("No error has been found")
    # what was there before reads as before: the reports recorded from `mc` as it was before it knew these properties
    import json
    recorded = json.loads((ROOT / "tests" / "golden" / "liveprops_mc_reports.json").read_text())
    p = run_mc(livegraph.DIR / "spin_flag_unfair.tla")
    assert p.returncode == 13 and p.stdout == recorded["spin_flag_unfair"]
    p = run_mc(ROOT / "specs" / "pluscal" / "peterson.tla")
    assert p.returncode == 0 and p.stdout == recorded["peterson"]


def code_of(amd, call):  # noqa: F811
    with pytest.raises(amd.McError) as e:
        call()
    return e.value.code


def test_errors(amd):  # noqa: F811
    prog, _ = reference("reach_mask")
    lp = prog.live_properties[0]
    eng = amd.Engine("pcal", prog.params, **KW)
    try:
        assert code_of(amd, lambda: eng.check_property(prog.fair_mask, lp)) == MC_ESTATE     # before a run
        assert code_of(amd, lambda: eng.predicates(1)) == MC_ESTATE
        assert code_of(amd, lambda: eng.check_components(1)) == MC_ESTATE
        assert eng.run().verdict == "ok"
        assert eng.check_property(prog.fair_mask, lp).violated == 0
        assert code_of(amd, lambda: eng.check_property(prog.fair_mask, dict(lp, q=3))) == MC_EBADCFG   # a predicate the program does not have
        assert code_of(amd, lambda: eng.check_property(prog.fair_mask, dict(lp, p=-1))) == MC_EBADCFG
        assert code_of(amd, lambda: eng.check_property(prog.fair_mask, dict(lp, kind=4))) == MC_EBADCFG
        assert code_of(amd, lambda: eng.check_property(prog.fair_mask, dict(lp, refused=True, reason="x"))) == MC_EBADCFG
        assert code_of(amd, lambda: eng.check_property(1 << 5, lp)) == MC_EBADCFG              # an instance the program does not have
        assert eng.check_property(prog.fair_mask, prog.live_properties[1]).violated == 1       # (none of that spoilt the engine)
        assert eng.liveness(prog.fair_mask).violated == 1 and eng.liveness_trace()[1]          # Termination after a property check: its own trace
        assert code_of(amd, lambda: eng.check_components(1)) == MC_ESTATE                      # ... and no property check to read the components of
        eng.step(1)                                                                            # a step releases the graph and what hangs on it
        assert code_of(amd, lambda: eng.check_property(prog.fair_mask, lp)) == MC_ESTATE
        assert code_of(amd, lambda: eng.liveness_trace()) == MC_ESTATE
        eng.simulate(4, depth=5, seed=1)
        assert code_of(amd, lambda: eng.check_property(prog.fair_mask, lp)) == MC_ESTATE       # after simulate
    finally:
        eng.close()
    # an evaluation error inside a predicate is the check's error, with the predicate and the least state it fails in: never a verdict
    bad = liveprops.compiled("pred_error")
    for jit in (False, True):
        eng = amd.Engine("pcal", bad.params, jit=jit, **KW)
        try:
            assert eng.run().verdict == "ok"
            texts = eng.state_texts(0, 3)
            assert "x = 2" in texts[2]
            for call in (lambda: eng.check_property(bad.fair_mask, bad.live_properties[0]), lambda: eng.predicates(3)):
                with pytest.raises(amd.McError) as e:
                    call()
                assert e.value.code == MC_ESTATE and "`( arr [ x ] = 5 )`" in str(e.value) and "in state 2 " in str(e.value), str(e.value)
            assert code_of(amd, lambda: eng.liveness_trace()) == MC_ESTATE
            assert eng.liveness(bad.fair_mask).violated == 0                                   # (Termination needs no predicate)
        finally:
            eng.close()
    bad.close()
    spec, params, _, deadlock = model(amd, "raft2")
    raft = amd.Engine(spec, params, deadlock=deadlock, **KW)
    try:
        assert raft.run().verdict == "ok"
        assert code_of(amd, lambda: raft.check_property(0, lp)) == MC_ENOSPEC
        assert code_of(amd, lambda: raft.predicates(1)) == MC_ENOSPEC
    finally:
        raft.close()
    sharded = amd.Engine("atomic_add", [3], shard_rank=0, shard_count=2, **KW)
    try:
        assert code_of(amd, lambda: sharded.check_property(prog.fair_mask, lp)) == MC_EBADCFG
        assert code_of(amd, lambda: sharded.predicates(1)) == MC_EBADCFG
    finally:
        sharded.close()
