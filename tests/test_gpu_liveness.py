"""Strongly connected components of the state graph on the device (mc_engine_scc) and `Termination` under weak process fairness
(mc_engine_liveness, mc_engine_liveness_trace, `mc X.tla` with PROPERTY Termination), against references that share no code with the
engine: an iterative Tarjan over the arrays Engine.graph() returns, and tests/livegraph.py (oracle/tla_eval.py over the translation)."""
import numpy as np
import pytest

import helpers
import livegraph
from test_gpu_coverage import KW, amd, model  # noqa: F401  (amd: the fixture)
from test_gpu_graph import run_mc

pytestmark = pytest.mark.gpu
ROOT = helpers.ROOT
MC_EBADCFG, MC_ENOSPEC, MC_ESTATE = -1, -9, -7
PETERSON = livegraph.Model(ROOT / "specs" / "pluscal" / "peterson.tla", ROOT / "specs" / "pluscal" / "peterson.cfg", {}, ["Proc(0)", "Proc(1)"], True)
VIOLATED = [k for k, m in livegraph.MODELS.items() if m.violated]

_cache = {}


def reference(name):
    """(program, LiveGraph) of a model, built once and left unchanged"""
    if name not in _cache:
        if name == "peterson":
            import tla_rust_amd
            prog = tla_rust_amd.Program(PETERSON.tla.read_text(), PETERSON.cfg.read_text())
            _cache[name] = (prog, livegraph.LiveGraph(prog, PETERSON))
        elif name == "ring_1000":
            import tla_rust_amd
            m = livegraph.MODELS["ring"]._replace(cfg="ring_1000.cfg", constants={"N": 1000})
            prog = tla_rust_amd.Program((livegraph.DIR / m.tla).read_text(), (livegraph.DIR / m.cfg).read_text())
            _cache[name] = (prog, livegraph.LiveGraph(prog, m))
        else:
            _cache[name] = livegraph.load(name)
    return _cache[name]


def engine_for(amd, name, **kw):  # noqa: F811
    if name in ("raft2", "ssi2x2", "voting"):
        spec, params, _, deadlock = model(amd, name)
        return amd.Engine(spec, params, deadlock=deadlock, **KW, **kw), None
    prog, g = reference(name)
    return amd.Engine("pcal", prog.params, **KW, **kw), g


def tarjan_of(info, offsets, dst):
    off = offsets.astype(np.int64).tolist()
    d = dst.tolist()
    return np.array(livegraph.tarjan(info.states, lambda v: d[off[v]:off[v + 1]]), dtype=np.uint32)


HAND = ("raft2", "ssi2x2", "voting")   # lowerings without LiveProc (and without a second back end)
SCC_CASES = [(n, False) for n in ("peterson", "raft2", "ssi2x2", "voting", "ring_1000", "ring", "two_loops")] + \
            [(n, True) for n in ("peterson", "ring_1000", "ring", "two_loops")]


@pytest.mark.parametrize("name,jit", SCC_CASES, ids=[f"{n}-{'jit' if j else 'interpreter' if n not in HAND else 'lowering'}" for n, j in SCC_CASES])
def test_components_equal_tarjans(amd, name, jit):  # noqa: F811
    eng, g = engine_for(amd, name, **({"jit": True} if jit else {}))
    try:
        r = eng.run()
        assert r.verdict == "ok" and r.queue_left == 0
        info, offsets, dst, _ = eng.graph()
        si, scc = eng.scc()
        want = tarjan_of(info, offsets, dst)
        assert si.states == info.states == len(scc)
        assert np.array_equal(scc, want)                       # ids included: the least arena index of the component
        sizes = np.bincount(want, minlength=info.states)
        assert si.components == int((sizes > 0).sum()) and si.nontrivial == int((sizes > 1).sum()) and si.largest == int(sizes.max())
        print(name, dict(si))
        if name == "peterson":
            assert si.largest > 1
        if name in ("ring", "ring_1000"):
            n = 1000 if name == "ring_1000" else 65
            assert si.largest == n and si.nontrivial == 1       # one component: 4 workgroups of 256 (N = 1000), one past a wavefront (N = 65)
        if name == "two_loops":
            assert si.nontrivial == 3 and si.largest == 4   # the cycle modulo 4 (later states) feeds the two cycles modulo 2
        if g is not None:   # by state text against Tarjan on the evaluator's graph
            texts = [t.replace("\n", " ") for t in eng.state_texts(0, info.states)]
            assert sorted(texts) == sorted(g.texts)
            mine = {}
            for v, c in enumerate(scc.tolist()):
                mine.setdefault(c, set()).add(texts[v])
            assert {frozenset(m) for m in mine.values()} == g.partition()
        again, scc2 = eng.scc()                                  # a second build on the same engine: the same arrays
        assert np.array_equal(scc, scc2) and (again.components, again.nontrivial, again.largest) == (si.components, si.nontrivial, si.largest)
    finally:
        eng.close()


def code_of(amd, call):  # noqa: F811
    with pytest.raises(amd.McError) as e:
        call()
    return e.value.code


def test_release_and_refusals(amd):  # noqa: F811
    prog, _ = reference("two_loops")
    eng = amd.Engine("pcal", prog.params, **KW)
    try:
        assert code_of(amd, lambda: eng.liveness(prog.fair_mask)) == MC_ESTATE      # before a run
        assert code_of(amd, lambda: eng.scc_read(0, 1)) == MC_ESTATE
        assert eng.run().verdict == "ok"
        eng.scc()
        assert eng.liveness(prog.fair_mask).violated == 1
        assert code_of(amd, lambda: eng.liveness(1 << 5)) == MC_EBADCFG             # an instance the program does not have
        eng.step(1)                                                                 # a step releases the graph and what hangs on it
        assert code_of(amd, lambda: eng.scc_read(0, 1)) == MC_ESTATE
        assert code_of(amd, lambda: eng.liveness_trace()) == MC_ESTATE
        eng.simulate(4, depth=5, seed=1)
        assert code_of(amd, lambda: eng.liveness(prog.fair_mask)) == MC_ESTATE      # after simulate
    finally:
        eng.close()
    short = amd.Engine("pcal", prog.params, max_levels=2, **KW)
    try:
        assert short.run().verdict == "budget"
        assert code_of(amd, lambda: short.liveness(prog.fair_mask)) == MC_ESTATE    # a budget-stopped search: not the complete graph
        si, scc = short.scc()                                                       # ... whose components are to be had all the same
        assert si.states == len(scc)
    finally:
        short.close()
    spec, params, _, deadlock = model(amd, "raft2")
    raft = amd.Engine(spec, params, deadlock=deadlock, **KW)
    try:
        assert raft.run().verdict == "ok"
        assert code_of(amd, lambda: raft.liveness(0)) == MC_ENOSPEC
    finally:
        raft.close()
    sharded = amd.Engine("atomic_add", [3], shard_rank=0, shard_count=2, **KW)
    try:
        assert code_of(amd, lambda: sharded.liveness(prog.fair_mask)) == MC_EBADCFG
        assert code_of(amd, lambda: sharded.scc()) == MC_EBADCFG
    finally:
        sharded.close()


@pytest.mark.parametrize("jit", [False, True], ids=["interpreter", "jit"])
@pytest.mark.parametrize("name", list(livegraph.MODELS))
def test_verdict_and_fair_components(amd, name, jit):  # noqa: F811
    prog, g = reference(name)
    want = g.fair_components(prog.fair_mask)
    assert bool(want) == livegraph.MODELS[name].violated
    eng = amd.Engine("pcal", prog.params, jit=jit, **KW)
    try:
        assert eng.run().verdict == "ok"
        li = eng.liveness(prog.fair_mask)
        print(name, jit, dict(li))
        assert li.violated == (1 if want else 0) and li.fair_components == len(want)
        if want:
            texts = [t.replace("\n", " ") for t in eng.state_texts(0, len(g.texts))]
            _, scc = eng.scc()
            chosen = frozenset(texts[v] for v in np.nonzero(scc == li.root)[0].tolist())
            assert chosen in want and li.root_size == len(chosen)
            # the least root = the fair component closest to the initial states: no other fair component holds an earlier state
            first = {c: min(texts.index(t) for t in c) for c in want}
            assert first[chosen] == min(first.values()) == li.root
            assert eng.liveness(prog.fair_mask).violated == 1   # (the components were rebuilt above: the check runs again on them)
    finally:
        eng.close()


@pytest.mark.parametrize("jit", [False, True], ids=["interpreter", "jit"])
@pytest.mark.parametrize("name", VIOLATED)
def test_counterexample(amd, name, jit):  # noqa: F811
    prog, g = reference(name)
    eng = amd.Engine("pcal", prog.params, jit=jit, **KW)
    try:
        r = eng.run()
        li = eng.liveness(prog.fair_mask)
        assert li.violated == 1
        prefix, cycle = eng.liveness_trace()
        assert (prefix, cycle) == eng.liveness_trace()                       # deterministic
        info, offsets, dst, _ = eng.graph()   # (rebuilds the graph: the trace above was read first)
        off = offsets.astype(np.int64).tolist()
        row = lambda v: dst[off[v]:off[v + 1]].tolist()  # noqa: E731
        assert prefix[0] < info.init_states                                   # starts at an initial state
        for u, v in zip(prefix, prefix[1:]):
            assert v in row(u)                                               # every step is an edge of graph()
        texts = [t.replace("\n", " ") for t in eng.state_texts(0, info.states)]
        fair = {p for p in range(g.nproc) if prog.fair_mask >> p & 1}
        stay = prefix[-1]
        if name in ("handoff_unfair",):
            assert cycle == [] and prefix == [0]                             # stuttering in the first state
        if not cycle:
            assert not g.done[g.index[texts[stay]]] and not (fair & g.en[g.index[texts[stay]]])   # every fair process is disabled there
            return
        assert cycle[0] == stay                                              # the prefix ends where the cycle starts
        walk = cycle + [cycle[0]]
        for u, v in zip(walk, walk[1:]):
            assert v in row(u) and u != v                                    # closed, along edges
        on = [g.index[texts[v]] for v in cycle]
        assert not any(g.done[i] for i in on)                                # no state on it is Done
        taken = set()
        for a, b in zip(on, on[1:] + on[:1]):
            taken |= {p for p, j in g.edges[a] if p >= 0 and j == b and j != a}
        disabled = set()
        for i in on:
            disabled |= set(range(g.nproc)) - g.en[i]
        assert fair <= (taken | disabled), (fair, taken, disabled)           # the cycle itself meets the fairness condition
        if name == "spin_flag_unfair":
            assert len(cycle) == 2
        if name == "ring":
            assert len(cycle) == 65
        assert r.verdict == "ok"
    finally:
        eng.close()


def test_mc_reports_termination(amd):  # noqa: F811
    import re
    p = run_mc(livegraph.DIR / "spin_flag_unfair.tla")
    assert p.returncode == 13, (p.returncode, p.stdout, p.stderr)
    out = p.stdout
    assert "Error: Temporal properties were violated." in out and "Error: The following behavior constitutes a counter-example:" in out
    assert "No error has been found" not in out
    numbers = [int(k) for k in re.findall(r"^State (\d+):", out, flags=re.M)]
    assert numbers == list(range(1, len(numbers) + 1)) and numbers
    back = re.findall(r"^Back to state (\d+): <(\w+)>$", out, flags=re.M)
    assert len(back) == 1 and 1 <= int(back[0][0]) <= len(numbers) and back[0][1] in ("Check", "Again")
    assert out.index("Back to state") > out.rindex("State %d:" % numbers[-1])
    p = run_mc(livegraph.DIR / "spin_flag.tla")
    assert p.returncode == 0 and "No error has been found" in p.stdout and "Temporal" not in p.stdout and "NOT checked" not in p.stdout
    p = run_mc(livegraph.DIR / "handoff_unfair.tla")
    assert p.returncode == 13 and re.search(r"^State 2: Stuttering$", p.stdout, flags=re.M)
    for stem, word in livegraph.REFUSED.items():
        p = run_mc(livegraph.DIR / (stem + ".tla"))
        assert p.returncode == 0, (stem, p.stdout, p.stderr)
        warn = [ln for ln in p.stdout.splitlines() if "NOT checked" in ln]
        assert len(warn) == 1 and warn[0].startswith("Warning: temporal property Termination NOT checked:") and word in warn[0]
        assert p.stdout.index("NOT checked") < p.stdout.index("No error has been found")
    p = run_mc(ROOT / "specs" / "pluscal" / "peterson.tla")
    assert p.returncode == 0 and "No error has been found" in p.stdout
    for new in ("Temporal", "NOT checked", "Back to state", "Stuttering", "counter-example"):
        assert new not in p.stdout



def test_a_sharded_mc_names_the_property_as_not_checked(amd):  # noqa: F811
    """`mc X.tla -gpus 2`: a sharded search keeps no state graph in one place, so the cfg's Termination is named before the verdict"""
    from test_gpu_sharded import _fake_env, _mc
    p = _mc(livegraph.DIR / "handoff_unfair.tla", "-gpus", 2, "-samedevice", env=_fake_env())
    assert p.returncode == 0, (p.stdout[-800:], p.stderr[-800:])
    warn = [ln for ln in p.stdout.splitlines() if "NOT checked" in ln]
    assert len(warn) == 1 and warn[0].startswith("Warning: temporal property Termination NOT checked:") and "sharded" in warn[0]
    assert p.stdout.index("NOT checked") < p.stdout.index("No error has been found")
    q = _mc(ROOT / "specs" / "pluscal" / "peterson.tla", "-gpus", 2, "-samedevice", env=_fake_env())
    assert q.returncode == 0 and "NOT checked" not in q.stdout
