"""The safety parts of a cfg PROPERTY of compiled PlusCal programs on the device: every model of specs_actprop/ on
the interpreter — and ap_seen and the violated ap_kinds as generated code — against tests/actprop.py (oracle/tla_eval.py over the
translation and a BFS written there): verdict, the violated PROPERTY, depth, the behaviour and its last step, and the states per level of
the models that hold.  Then -simulate, -continue and `mc` itself."""
import pytest

import actprop
import helpers
from test_gpu_coverage import KW, amd  # noqa: F401  (amd: the fixture)
from test_gpu_graph import run_mc

pytestmark = pytest.mark.gpu


def check_run(amd, name, jit=False):  # noqa: F811
    prog, ref, want = actprop.load(name)
    eng = amd.Engine("pcal", prog.params, jit=jit, **KW)
    try:
        r = eng.run()
        got = dict(distinct=r.distinct, generated=r.generated, depth=r.depth, verdict=r.verdict, trace_len=r.trace_len, levels=list(r.levels))
        print(name, jit, got, r.violated_invariant)
        expect = {k: want[k] for k in got}
        if want["trace_len"] == 1:   # broken by an initial state: mc_result.trace_len is 0 there, for an INVARIANT too (the engine's convention:
            expect["trace_len"] = 0  # no stored state leads to it); the behaviour mc_engine_trace returns has the one state, checked below
        assert got == expect, name
        if want["verdict"] == "ok":
            texts = [t.replace("\n", " ") for t in eng.state_texts(0, r.distinct)]
            at, lines = 0, []
            for n in r.levels:   # the arena holds the states level by level
                lines.append(sorted(texts[at:at + n]))
                at += n
            assert lines == want["level_lines"], name
            return
        assert prog.invariant(r.violated_invariant) == want["violated"], name
        by_index = {a.index: a for a in prog.action_properties}
        ninv = len(ref.invariants) + sum(a.kind == "always" for a in prog.action_properties)
        tr = [(a, t.replace("\n", " ")) for a, t in eng.trace()]
        assert len(tr) == want["trace_len"]
        if want["last_step"]:   # a property of a step: an index behind the invariants', and the last two states are the offending step
            assert r.violated_invariant >= ninv and by_index[r.violated_invariant].kind == "step"
            assert (tr[-2][1], tr[-1][1]) == want["last_step"] and ref.breaks(want["violated"], tr[-2][1], tr[-1][1])
        elif want["trace_len"] == 1 and want["violated"] not in ref.invariants:   # an initial predicate
            assert r.violated_invariant >= ninv and by_index[r.violated_invariant].kind == "init"
        else:                   # an INVARIANT or a `[]P`: the last state breaks it
            assert r.violated_invariant < ninv and tr[-1][1] in want["state_violations"][want["violated"]]
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(actprop.MODELS))
def test_every_model_equals_the_reference(amd, name):  # noqa: F811
    check_run(amd, name)


@pytest.mark.parametrize("name", ["ap_seen", "ap_kinds_bad"])
def test_generated_code_equals_the_reference(amd, name):  # noqa: F811
    class Handle:
        h = actprop.load(name)[0].params[0]
    assert "run_aprop" in helpers.program_codegen(Handle)
    check_run(amd, name, jit=True)


@pytest.mark.parametrize("walks", [1, 65])
def test_a_simulated_walk_ends_at_the_property(amd, walks):  # noqa: F811
    """ap_monotone: six steps per walk and x stays within 0..4 from 2, so every walk that runs to its end steps down at least twice: the
    first such step ends it, and the behaviour it leaves ends in the offending step"""
    prog, ref, want = actprop.load("ap_monotone")
    eng = amd.Engine("pcal", prog.params, **KW)
    try:
        r = eng.simulate(walks, depth=12, seed=7)
        assert r.verdict == "invariant" and prog.invariant(r.violated_invariant) == "Mono", dict(r)
        tr = [t.replace("\n", " ") for _, t in eng.trace()]
        assert len(tr) == r.trace_len >= 2 and ref.breaks("Mono", tr[-2], tr[-1])
        assert not any(ref.breaks("Mono", a, b) for a, b in zip(tr[:-2], tr[1:-1]))   # (the first offending step ends the walk)
    finally:
        eng.close()


def test_continue_lists_the_property_last_and_fatal(amd):  # noqa: F811
    prog, ref, want = actprop.load("ap_two")
    eng = amd.Engine("pcal", prog.params, keep_going=True, **KW)
    try:
        r = eng.run()
        assert (r.verdict, prog.invariant(r.violated_invariant), r.depth) == ("invariant", "Inv", 2)
        rows = eng.violations()
        print([dict(v) for v in rows])
        inv, last = rows[0], rows[-1]
        assert (inv.name, inv.states, inv.outside, inv.fatal) == ("Inv", len(want["state_violations"]["Inv"]), 0, False)
        assert last.fatal and (last.kind, last.name) == ("invariant", "KeepY") and last.outside == len(want["step_violations"]["KeepY"]) == 1
        assert [v.name for v in rows[:-1]] == ["Inv", "Deadlock"] or [v.name for v in rows[:-1]] == ["Inv"]   # (no row for a property of a step)
        tr = [t.replace("\n", " ") for _, t in eng.violation_trace(len(rows) - 1)]
        assert len(tr) == 2 and ref.breaks("KeepY", tr[0], tr[1])
    finally:
        eng.close()


def test_mc_reports_the_properties(amd):  # noqa: F811
    p = run_mc(actprop.DIR / "ap_monotone.tla")
    assert p.returncode == 12, (p.returncode, p.stdout, p.stderr)
    assert "Error: Action property Mono is violated." in p.stdout and "NOT checked" not in p.stdout, p.stdout
    assert "State 2:" in p.stdout and "State 3:" not in p.stdout and "/\\ x = 1" in p.stdout
    p = run_mc(actprop.DIR / "ap_spec.tla")
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    warn = [ln for ln in p.stdout.splitlines() if "NOT checked" in ln]
    assert len(warn) == 1 and "HSpec" in warn[0] and "WF_hv ( HNext )" in warn[0] and "No error has been found" in p.stdout, p.stdout
    p = run_mc(actprop.DIR / "ap_spec.tla", "-config", actprop.DIR / "ap_spec_badinit.cfg")
    assert p.returncode == 12 and "Error: Action property HSpecOne is violated." in p.stdout and "State 2:" not in p.stdout, p.stdout
    p = run_mc(actprop.DIR / "ap_mixed.tla")   # both halves are decided: the step formula by the search, `~>` on the state graph
    assert p.returncode == 0 and "NOT checked" not in p.stdout and "No error has been found" in p.stdout, (p.returncode, p.stdout, p.stderr)
    p = run_mc(actprop.DIR / "ap_always.tla")
    assert p.returncode == 12 and "Error: Invariant Small is violated." in p.stdout and "NOT checked" not in p.stdout, p.stdout
    q = run_mc(actprop.DIR / "ap_always.tla", "-config", actprop.DIR / "ap_always_inv.cfg")
    strip = lambda s: [ln for ln in s.splitlines() if "seconds" not in ln and "Finished in" not in ln]   # noqa: E731
    assert q.returncode == 12 and strip(q.stdout.replace("Le3", "Small")) == strip(p.stdout), (p.stdout, q.stdout)
