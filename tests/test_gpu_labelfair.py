"""Liveness under fairness label by label on the device (mc_program_fairness_units, mc_engine_liveness_units,
mc_engine_liveness_check_units, k_live_unit's array, the counterexample of mc_engine_liveness_trace, `mc X.tla -labelfair`), interpreter
and generated code, against tests/labelfair.py — oracle/tla_eval.py over the translation, every conjunct's own text evaluated as an
action, and the rule of tests/unitfair.py — by state text; the least-index rules of the engine are the reference's under the engine's own
order of the states."""
import re

import numpy as np
import pytest

import helpers
import labelfair
import livegraph
import liveprops
import strongfair
import unitfair
from test_gpu_coverage import KW, amd  # noqa: F401  (amd: the fixture)
from test_gpu_graph import run_mc

pytestmark = pytest.mark.gpu
ROOT = helpers.ROOT
MC_EBADCFG, MC_ESTATE = -1, -7
BACKENDS = pytest.mark.parametrize("jit", [False, True], ids=["interpreter", "jit"])

_refs = {}


def reference(name):
    """(program, UnitGraph, checks) of a model, built once and left unchanged"""
    if name not in _refs:
        _refs[name] = labelfair.load(name)
    return _refs[name]


class Run:
    """one finished search per (model, back end), shared by the tests"""

    def __init__(self, amd, name, jit):  # noqa: F811
        self.prog, self.g, self.checks = reference(name)
        self.fu, self.texts_conj, why = self.prog.fairness_units
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
        return labelfair.decide_model(self.g, prop, rank=self.rank)

    def ask(self, prop):
        if prop["kind"] == strongfair.TERMINATION:
            return self.eng.liveness_units(self.fu)
        return self.eng.check_property_units(self.fu, prop)

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
    """a path of the oracle's graph from an initial state into ONE final component, then a closed walk inside it that meets every
    conjunct by the reference's own membership; never a state the refinement closed"""
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
    on = [ref(v) for v in cycle]
    assert set(on) <= set(want.root) and path[-1] in want.root
    if cycle:
        assert cycle[0] == prefix[-1] and all(a != b for a, b in zip(on, on[1:] + on[:1]))
    wrong = unitfair.cycle_meets_every_conjunct(g.uedges, g.of_unit, g.nconj, g.weak, g.strong, on, path[-1])
    assert wrong is None, wrong
    states = on or [path[-1]]
    assert all(M[i] for i in states) and any(T[i] for i in states)


@BACKENDS
@pytest.mark.parametrize("name", list(labelfair.MODELS))
def test_every_check_equals_the_reference(runs, name, jit):
    r = runs(name, jit)
    assert {c for c, _ in r.checks} == set(labelfair.MODELS[name].expect)
    for cname, prop in r.checks:
        want = r.want(prop)
        info, si = r.ask(prop)
        print(name, cname, "jit" if jit else "interpreter", dict(info), dict(si))
        assert info.violated == (1 if want.violated else 0) == (1 if labelfair.MODELS[name].expect[cname] else 0)
        assert info.fair_components == si.final_components == len(want.final)
        assert (si.rounds, si.closed_states, si.scc_builds) == (want.rounds, want.closed, want.rounds - 1)
        if prop["kind"] != strongfair.TERMINATION:
            assert (info.mask_states, info.bad_starts) == (want.mask_states, want.bad_starts)
        if want.violated:
            if prop["kind"] == strongfair.TERMINATION:
                assert info.root == r.rank[want.first_root]
            else:
                assert info.witness == r.rank[want.witness]
                assert info.root == min(r.arena(want.root))
            assert info.root_size == len(want.root)
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


@BACKENDS
@pytest.mark.parametrize("name", list(labelfair.MODELS))
def test_the_unit_of_every_edge_is_the_conjuncts_membership(runs, name, jit):
    """unit[] as k_live_unit<S> wrote it: for every edge i -> j the conjuncts of its unit are conjuncts that, by their own TLA+ text,
    have a step i -> j, and together the edges i -> j have all of them; the terminating disjunct's edge has unit -1"""
    r = runs(name, jit)
    _, offsets, dst, _ = r.eng.graph()                                # (a new graph build releases the units: the check comes after it)
    r.ask(r.checks[0][1])
    off, d = offsets.astype(np.int64).tolist(), dst.tolist()
    units = r.eng.edge_units(0, len(d)).tolist()
    g = r.g
    seen_two = False
    for i in range(r.n):
        gi = g.index[r.texts[i]]
        by_target = {}
        for e in range(off[i], off[i + 1]):
            u = units[e]
            if u < 0:
                assert d[e] == i and g.done[gi]
                continue
            assert u < r.fu.nunits
            ks = {k for k in range(r.fu.nconj) if r.fu.of_unit[u] >> k & 1}
            seen_two |= len(ks) == 2
            by_target.setdefault(d[e], set()).update(ks)
            assert ks <= g.members(gi, g.index[r.texts[d[e]]]), (r.texts[i], r.texts[d[e]], ks)
        for j, ks in by_target.items():
            assert ks == g.members(gi, g.index[r.texts[j]]), (r.texts[i], r.texts[j], ks)
    if name in ("lock_plus", "toggle_plus"):
        assert seen_two                                               # a `+` label's unit is in its process's WF conjunct and in its own SF one


def test_the_report_with_plus_under_fair_plus_equals_the_one_without(amd):  # noqa: F811
    a, b = run_mc(labelfair.DIR / "fairplus_plus.tla", "-labelfair"), run_mc(labelfair.DIR / "fairplus_plain.tla", "-labelfair")
    assert a.returncode == b.returncode == 0
    assert a.stdout.replace("fairplus_plus", "X") == b.stdout.replace("fairplus_plain", "X")


def test_errors(amd):  # noqa: F811
    prog, _, checks = reference("lock_plus")
    fu, _, _ = prog.fairness_units
    lp = checks[0][1]
    eng = amd.Engine("pcal", prog.params, **KW)
    F = type(fu)
    table = [fu.of_unit[u] for u in range(fu.nunits)]

    def code_of(call):
        with pytest.raises(amd.McError) as e:
            call()
        return e.value.code
    try:
        assert code_of(lambda: eng.liveness_units(fu)) == MC_ESTATE                                                        # before a run
        assert eng.run().verdict == "ok"
        assert code_of(lambda: eng.edge_units(0, 1)) == MC_ESTATE                                                          # before a check by units
        assert code_of(lambda: eng.liveness_units(F.make(table, fu.nconj, fu.weak_mask | fu.strong_mask, fu.strong_mask))) == MC_EBADCFG   # overlap
        assert code_of(lambda: eng.liveness_units(F.make(table, fu.nconj, fu.weak_mask, fu.strong_mask | 1 << fu.nconj))) == MC_EBADCFG   # a bit >= nconj
        assert code_of(lambda: eng.liveness_units(F.make([m | 1 << 40 for m in table], fu.nconj, fu.weak_mask, fu.strong_mask))) == MC_EBADCFG
        assert code_of(lambda: eng.liveness_units(F.make(table, 65, fu.weak_mask, fu.strong_mask))) == MC_EBADCFG          # counts out of range
        assert code_of(lambda: eng.liveness_units(F.make(table, fu.nconj, fu.weak_mask, fu.strong_mask, nunits=128))) == MC_EBADCFG
        assert code_of(lambda: eng.liveness_units(F.make(table[:1], fu.nconj, fu.weak_mask, fu.strong_mask))) == MC_EBADCFG  # fewer units than the program's
        assert code_of(lambda: eng.check_property_units(fu, dict(lp, kind=4))) == MC_EBADCFG
        assert eng.check_property_units(fu, lp)[0].violated == 0                                                           # (none of that spoilt the engine)
        assert eng.check_components(1).tolist() == [0]
    finally:
        eng.close()


def test_mc_without_the_option_is_unchanged(amd):  # noqa: F811
    """what `mc` said before it knew the label modifiers: the refusal lines, with and without -strongfair"""
    D = labelfair.DIR
    for stem in ("lock_plus", "spin_minus", "two_labels_minus", "toggle_plus", "treiber_procs", "rec_fair"):
        for opts in ((), ("-strongfair",)):
            p = run_mc(D / (stem + ".tla"), *opts)
            assert p.returncode == 0, (stem, p.stdout, p.stderr)
            warn = [ln for ln in p.stdout.splitlines() if "NOT checked" in ln]
            assert warn and all("modifier" in ln or "procedures" in ln for ln in warn) and "No error has been found" in p.stdout
    p = run_mc(D / "fairplus_plus.tla")
    assert len([ln for ln in p.stdout.splitlines() if "NOT checked" in ln and "fair+" in ln]) == 1
    p = run_mc(D / "uni_minus.tla")                                       # a `--fair algorithm` module goes where it went without the option
    assert p.returncode != 0 and "not a lowered spec" in p.stderr
    p = run_mc("-help")
    assert "-labelfair" in p.stderr


def test_mc_labelfair_checks_the_label_modifiers(amd):  # noqa: F811
    D = labelfair.DIR
    for stem in ("lock_plus", "spin_fair", "toggle_plus", "fairplus_plus", "fairplus_plain", "treiber_procs", "lock_proc", "rec_fair"):
        p = run_mc(D / (stem + ".tla"), "-labelfair")
        assert p.returncode == 0 and "No error has been found" in p.stdout, (stem, p.stdout, p.stderr)
        for new in ("Temporal", "NOT checked", "Back to state", "Stuttering", "counter-example"):
            assert new not in p.stdout, (stem, new)
    for stem in ("lock_weak", "spin_minus", "two_labels_minus", "unfair_plus", "uni_minus", "proc_minus"):
        p = run_mc(D / (stem + ".tla"), "-labelfair")
        assert p.returncode == 13, (stem, p.returncode, p.stdout, p.stderr)
        assert "Error: Temporal properties were violated." in p.stdout and "NOT checked" not in p.stdout
        numbers = [int(k) for k in re.findall(r"^State (\d+):", p.stdout, flags=re.M)]
        assert numbers == list(range(1, len(numbers) + 1)) and numbers
    p = run_mc(D / "two_labels_minus.tla", "-labelfair")                  # a cycle: the Spinner spins while the Setter rests at `idle`
    back = re.findall(r"^Back to state (\d+): <(\w+)>$", p.stdout, flags=re.M)
    assert len(back) == 1 and back[0][1] == "spin"
    for stem in ("spin_minus", "uni_minus"):                              # no cycle: the behaviour stutters at the `-` label
        p = run_mc(D / (stem + ".tla"), "-labelfair")
        assert re.search(r"^State \d+: Stuttering$", p.stdout, flags=re.M)


def test_mc_labelfair_changes_nothing_else(amd):  # noqa: F811
    """a program with none of these forms: the report is byte for byte the one without the option; the other refusals stay"""
    S = strongfair.DIR
    for tla in (S / "sem2_fair.tla", S / "toggle_fair.tla", liveprops.DIR / "peterson_loop.tla", liveprops.DIR / "stable.tla",
                livegraph.DIR / "handoff.tla", livegraph.DIR / "spin_flag_unfair.tla"):
        a, b = run_mc(tla), run_mc(tla, "-labelfair")
        assert (a.returncode, a.stdout) == (b.returncode, b.stdout), tla
    for tla in (S / "sem2_strong.tla", S / "subcycle.tla", S / "leftover.tla"):   # `fair+` alone: -strongfair's report
        a, b = run_mc(tla, "-strongfair"), run_mc(tla, "-labelfair")
        assert (a.returncode, a.stdout) == (b.returncode, b.stdout), tla
    p = run_mc(livegraph.DIR / "refused_procedure.tla")                   # procedures: refused without the option, checked with it
    warn = [ln for ln in p.stdout.splitlines() if "NOT checked" in ln]
    assert p.returncode == 0 and len(warn) == 1 and "procedures" in warn[0]
    p = run_mc(livegraph.DIR / "refused_procedure.tla", "-labelfair")
    assert p.returncode == 0 and "NOT checked" not in p.stdout and "No error has been found" in p.stdout
    p = run_mc(labelfair.DIR / "lock_plus.tla", "-labelfair", "-maxdistinct", "3")
    assert "NOT checked" in p.stdout and "did not finish" in p.stdout
