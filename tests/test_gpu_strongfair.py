"""Liveness of `fair+` PlusCal algorithms on the device (mc_program_fairness_strong, mc_engine_liveness_strong,
mc_engine_liveness_check_strong, the counterexample of mc_engine_liveness_trace, `mc X.tla -strongfair`), interpreter and generated code,
against tests/strongfair.py — oracle/tla_eval.py over the translation and the rule restated from DESIGN.md section 19 — by state text;
the least-index rules of the engine are the reference's under the engine's own order of the states."""
import re

import numpy as np
import pytest

import helpers
import livegraph
import liveprops
import strongfair
from test_gpu_coverage import KW, amd  # noqa: F401  (amd: the fixture)
from test_gpu_graph import run_mc

pytestmark = pytest.mark.gpu
ROOT = helpers.ROOT
MC_EBADCFG, MC_ESTATE = -1, -7
BACKENDS = pytest.mark.parametrize("jit", [False, True], ids=["interpreter", "jit"])

_refs = {}


def reference(name):
    """(program, StrongGraph, checks) of a model, built once and left unchanged"""
    if name not in _refs:
        _refs[name] = strongfair.load(name)
    return _refs[name]


class Run:
    """one finished search per (model, back end), shared by the tests"""

    def __init__(self, amd, name, jit):  # noqa: F811
        self.prog, self.g, self.checks = reference(name)
        self.weak, self.strong, why = self.prog.strong_fairness
        assert why is None
        self.eng = amd.Engine("pcal", self.prog.params, jit=jit, **KW)
        r = self.eng.run()
        assert r.verdict == "ok" and r.queue_left == 0
        self.n = r.distinct
        self.texts = [t.replace("\n", " ") for t in self.eng.state_texts(0, self.n)]
        assert sorted(self.texts) == sorted(self.g.texts)
        self.at = {t: i for i, t in enumerate(self.texts)}          # state text -> arena index
        self.rank = [self.at[t] for t in self.g.texts]               # reference number -> arena index

    def want(self, prop):
        return strongfair.decide_model(self.g, prop, self.weak, self.strong, rank=self.rank)

    def ask(self, prop):
        """(the check's info, mc_live_strong_info) from the engine"""
        if prop["kind"] == strongfair.TERMINATION:
            return self.eng.liveness_strong(self.weak, self.strong)
        return self.eng.check_property_strong(self.weak, self.strong, prop)

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


def check_counterexample(r, prop, want, info, prefix, cycle):
    """a path of the oracle's graph from an initial state into ONE final component, then a closed walk inside it that is fair by the
    rule on its own states and holds a T state; never a state the refinement closed"""
    g = r.g
    ref = lambda v: g.index[r.texts[v]]   # noqa: E731  (arena index -> the reference's number)
    M, S, T = strongfair.sets(prop, g.bits, len(g.init), g.done)
    path = [ref(v) for v in prefix]
    assert path[0] in g.init
    for u, v in zip(path, path[1:]):
        assert any(j == v for _, j in g.edges[u])
    if prop["kind"] != strongfair.TERMINATION:
        w = prefix.index(info.witness)
        assert S[path[w]] and all(M[v] for v in path[w:])
        assert prefix[w:] == [r.rank[v] for v in want.path]
    on = [ref(v) for v in cycle] or [path[-1]]
    assert set(on) <= set(want.root) and path[-1] in want.root
    if cycle:
        assert cycle[0] == prefix[-1]
        for a, b in zip(on, on[1:] + on[:1]):
            assert a != b and any(j == b for _, j in g.edges[a])
    taken = set()
    for a, b in zip(on, on[1:] + on[:1]) if cycle else []:
        taken |= {p for p, j in g.edges[a] if p >= 0 and j == b and j != a}
    disabled = set().union(*[set(range(g.nproc)) - g.en[i] for i in on])
    enabled = set().union(*[g.en[i] for i in on])
    W, F = ({p for p in range(g.nproc) if m >> p & 1} for m in (r.weak, r.strong))
    assert W <= taken | disabled and F & enabled <= taken, (W, F, taken, disabled, enabled)
    assert all(M[i] for i in on) and any(T[i] for i in on)


@BACKENDS
@pytest.mark.parametrize("name", list(strongfair.MODELS))
def test_every_check_equals_the_reference(runs, name, jit):
    r = runs(name, jit)
    assert {c for c, _ in r.checks} == set(strongfair.MODELS[name].expect)
    for cname, prop in r.checks:
        want = r.want(prop)
        info, si = r.ask(prop)
        print(name, cname, "jit" if jit else "interpreter", dict(info), dict(si))
        assert info.violated == (1 if want.violated else 0) == (1 if strongfair.MODELS[name].expect[cname] else 0)
        assert info.fair_components == si.final_components == len(want.final)
        assert (si.rounds, si.closed_states, si.scc_builds) == (want.rounds, want.closed, want.rounds - 1)
        if name in strongfair.ROUNDS:
            assert si.rounds == strongfair.ROUNDS[name]
        if prop["kind"] != strongfair.TERMINATION:
            assert (info.mask_states, info.bad_starts) == (want.mask_states, want.bad_starts)
        if want.violated:
            if prop["kind"] == strongfair.TERMINATION:
                assert info.root == r.rank[want.first_root]
            else:
                assert info.witness == r.rank[want.witness]
                assert info.root == min(r.arena(want.root))
            assert info.root_size == len(want.root)
        # the refined ids: a final component's least arena index on its states, every other state its own
        ids = r.eng.check_components(r.n).tolist()
        expect = list(range(r.n))
        for c in want.final:
            for v in c:
                expect[r.rank[v]] = min(r.arena(c))
        assert ids == expect
        if want.violated:
            prefix, cycle = r.eng.liveness_trace()
            assert (prefix, cycle) == r.eng.liveness_trace()          # deterministic
            check_counterexample(r, prop, want, info, prefix, cycle)
            if name == "subcycle":                                    # the printed cycle avoids every state where Exit is enabled
                assert cycle and not any(0 in r.g.en[r.g.index[r.texts[v]]] for v in cycle)
            if name == "leftover":                                    # a one-state final component: the behaviour stutters
                assert cycle == [] and info.root_size == 1
        again, si2 = r.ask(prop)
        assert {k: v for k, v in again.items() if k not in ("seconds", "scc_builds")} == {k: v for k, v in info.items() if k not in ("seconds", "scc_builds")}
        assert (si2.rounds, si2.closed_states, si2.final_components) == (si.rounds, si.closed_states, si.final_components)
    # the full graph's components are untouched
    scc = r.eng.scc_read(0, r.n)
    ginfo, offsets, dst, _ = r.eng.graph()
    off, d = offsets.astype(np.int64).tolist(), dst.tolist()
    assert np.array_equal(scc, np.array(livegraph.tarjan(ginfo.states, lambda v: d[off[v]:off[v + 1]]), dtype=np.uint32))


@pytest.mark.parametrize("name", ["sem2_strong", "toggle_strong", "subcycle"])
def test_strong_read_as_weak_and_the_weak_entry_agree(runs, name):
    """strong_mask = 0 on a model: every field of the weak call's info but `seconds`, and a weak check after a strong one reads as alone"""
    r = runs(name, False)
    both = r.weak | r.strong
    for cname, prop in r.checks:
        r.ask(prop)                                                   # a strong check first
        if prop["kind"] == strongfair.TERMINATION:
            a, (b, si) = r.eng.liveness(both), r.eng.liveness_strong(both, 0)
        else:
            a, (b, si) = r.eng.check_property(both, prop), r.eng.check_property_strong(both, 0, prop)
        drop = ("seconds", "scc_builds")
        assert {k: v for k, v in a.items() if k not in drop} == {k: v for k, v in b.items() if k not in drop}, cname
        assert si.rounds == 1 and si.scc_builds == 0
        want = strongfair.decide_model(r.g, prop, both, 0, rank=r.rank)
        assert a.violated == (1 if want.violated else 0)


RING = [("ring_strong", 65, 32), ("ring_strong_1000", 1000, 500)]


@BACKENDS
@pytest.mark.parametrize("cfg,n,half", RING, ids=[x[0] for x in RING])
def test_the_ring(amd, cfg, n, half, jit):  # noqa: F811
    """ring_cut's shape for the kernels at size: one component of n states blocked by the stopper; the first round closes the one state
    that enables it, the second round's build peels a path of n - 1 states, every one closed.  Under weak fairness: violated."""
    prog = strongfair.compiled("ring_strong", cfg)
    eng = amd.Engine("pcal", prog.params, jit=jit, **KW)
    try:
        r = eng.run()
        assert r.verdict == "ok" and r.queue_left == 0 and r.distinct == n + 2
        weak, strong, why = prog.strong_fairness
        assert (weak, strong, why) == (1, 2, None)
        (lp,) = [x for x in prog.live_properties if not x["refused"]]
        li, si = eng.liveness_strong(weak, strong)
        print(cfg, "jit" if jit else "interpreter", "Termination strong", dict(li), dict(si))
        assert li.violated == 0 and (si.rounds, si.scc_builds, si.closed_states, si.final_components) == (2, 1, n + 2, 0)
        assert eng.check_components(r.distinct).tolist() == list(range(r.distinct))
        ci, si = eng.check_property_strong(weak, strong, lp)
        print(cfg, "Stops strong", dict(ci), dict(si))
        assert ci.violated == 0 and ci.mask_states == n and (si.rounds, si.scc_builds, si.closed_states) == (2, 1, n)
        wl = eng.liveness(weak | strong)
        wc = eng.check_property(weak | strong, lp)
        print(cfg, "Termination weak", dict(wl), "Stops weak", dict(wc))
        assert wl.violated == 1 and wl.root_size == n and wc.violated == 1 and wc.root_size == n
        prefix, cycle = eng.liveness_trace()
        assert len(cycle) == n
    finally:
        eng.close()
        prog.close()


def test_errors(amd):  # noqa: F811
    prog, _, checks = reference("subcycle")
    weak, strong, _ = prog.strong_fairness
    lp = checks[1][1]
    eng = amd.Engine("pcal", prog.params, **KW)

    def code_of(call):
        with pytest.raises(amd.McError) as e:
            call()
        return e.value.code
    try:
        assert code_of(lambda: eng.liveness_strong(weak, strong)) == MC_ESTATE                  # before a run
        assert eng.run().verdict == "ok"
        assert code_of(lambda: eng.liveness_strong(weak | strong, strong)) == MC_EBADCFG        # overlapping masks
        assert code_of(lambda: eng.liveness_strong(weak, strong | 1 << 5)) == MC_EBADCFG        # an instance the program does not have
        assert code_of(lambda: eng.check_property_strong(weak | strong, strong, lp)) == MC_EBADCFG
        assert code_of(lambda: eng.check_property_strong(weak, strong, dict(lp, kind=4))) == MC_EBADCFG
        assert eng.liveness_strong(weak, strong)[0].violated == 1                               # (none of that spoilt the engine)
        assert eng.check_components(1).tolist() == [0]                                          # ... and the refined ids are served
        assert eng.liveness(weak | strong).violated == 1
        assert code_of(lambda: eng.check_components(1)) == MC_ESTATE                            # a weak Termination has none, as before
    finally:
        eng.close()


def test_mc_without_the_option_is_unchanged(amd):  # noqa: F811
    """what `mc` said before it knew strong fairness"""
    D = strongfair.DIR
    for stem in ("sem2_strong", "toggle_strong", "subcycle", "ring_strong"):
        p = run_mc(D / (stem + ".tla"))
        assert p.returncode == 0, (stem, p.stdout, p.stderr)
        warn = [ln for ln in p.stdout.splitlines() if "NOT checked" in ln]
        assert warn and all("fair+" in ln for ln in warn) and "No error has been found" in p.stdout
    p = run_mc(livegraph.DIR / "refused_strong.tla")
    assert p.returncode == 0 and len([ln for ln in p.stdout.splitlines() if "NOT checked" in ln and "fair+" in ln]) == 1
    p = run_mc("-help")
    assert "-strongfair" in p.stderr


def test_mc_strongfair_checks_fair_plus(amd):  # noqa: F811
    """checked, and reported in the existing layouts"""
    D = strongfair.DIR
    for stem in ("sem2_strong", "toggle_strong", "mixed_sf", "ring_strong"):
        p = run_mc(D / (stem + ".tla"), "-strongfair")
        assert p.returncode == 0 and "No error has been found" in p.stdout, (stem, p.stdout, p.stderr)
        for new in ("Temporal", "NOT checked", "Back to state", "Stuttering", "counter-example"):
            assert new not in p.stdout, (stem, new)
    p = run_mc(livegraph.DIR / "refused_strong.tla", "-strongfair")
    assert "NOT checked" not in p.stdout and p.returncode in (0, 13)
    p = run_mc(D / "subcycle.tla", "-strongfair")
    assert p.returncode == 13, (p.returncode, p.stdout, p.stderr)
    out = p.stdout
    assert "Error: Temporal properties were violated." in out and "NOT checked" not in out
    numbers = [int(k) for k in re.findall(r"^State (\d+):", out, flags=re.M)]
    assert numbers == list(range(1, len(numbers) + 1)) and numbers
    back = re.findall(r"^Back to state (\d+): <(\w+)>$", out, flags=re.M)
    assert len(back) == 1 and back[0][1] == "L"
    cyc = out[out.index(f"State {back[0][0]}:"):]
    assert "x = 2" not in cyc                                          # the cycle avoids the state where Exit is enabled
    p = run_mc(D / "leftover.tla", "-strongfair")
    assert p.returncode == 13 and re.search(r"^State \d+: Stuttering$", p.stdout, flags=re.M)
    for stem in ("mixed_wf", "mixed_noise"):
        p = run_mc(D / (stem + ".tla"), "-strongfair")
        assert p.returncode == 13, (stem, p.stdout, p.stderr)


def test_mc_strongfair_changes_nothing_else(amd):  # noqa: F811
    """a program without `fair+`: the report is byte for byte the one without the option; the other refusals stay"""
    D = strongfair.DIR
    for tla in (D / "sem2_fair.tla", D / "toggle_fair.tla", liveprops.DIR / "peterson_loop.tla", liveprops.DIR / "stable.tla"):
        a, b = run_mc(tla), run_mc(tla, "-strongfair")
        assert (a.returncode, a.stdout) == (b.returncode, b.stdout), tla
    assert run_mc(D / "sem2_fair.tla").returncode == 13 and run_mc(liveprops.DIR / "peterson_loop.tla", "-strongfair").returncode == 0
    # refusals that stay: a `+` label, a VIEW, an unfinished search
    for tla, word in ((D / "refused_strong_label.tla", "modifier"), (livegraph.DIR / "refused_label.tla", "modifier"),
                      (livegraph.DIR / "refused_procedure.tla", "procedures")):
        p = run_mc(tla, "-strongfair")
        warn = [ln for ln in p.stdout.splitlines() if "NOT checked" in ln]
        assert p.returncode == 0 and len(warn) == 1 and word in warn[0], (tla, p.stdout, p.stderr)
    p = run_mc(D / "ring_strong.tla", "-strongfair", "-maxdistinct", "10")
    assert "NOT checked" in p.stdout and "did not finish" in p.stdout
