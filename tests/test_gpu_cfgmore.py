"""cfg VIEW and ACTION_CONSTRAINT of compiled PlusCal programs on the device: every model of specs_cfgmore/ on the
interpreter — and ghost_history, ac_two and wide as generated code, by pairs and slot by slot, wide also with unpacked rows — against
tests/cfgmore.py (oracle/tla_eval.py over the translation and a BFS written there): counts, levels, verdict, trace length, and the SETS
OF VIEW VALUES per level (the representative of a view value is free).  Then the state graph, -coverage, -simulate, checkpoints and `mc`."""
import pytest

import cfgmore
import helpers
from test_gpu_coverage import KW, amd  # noqa: F401  (amd: the fixture)
from test_gpu_graph import run_mc

pytestmark = pytest.mark.gpu
ROOT = helpers.ROOT
GENERATED = ("ghost_history", "ac_two", "wide")
BACKENDS = {"interpreter": dict(jit=False), "pairs": dict(jit=True), "slots": dict(jit=True, debug_flags=32)}
CASES = [(n, "interpreter") for n in cfgmore.MODELS] + [(n, b) for n in GENERATED for b in ("pairs", "slots")]


def check_run(amd, name, backend):  # noqa: F811
    prog, ref, want = cfgmore.load(name)
    eng = amd.Engine("pcal", prog.params, **BACKENDS[backend], **KW)
    try:
        r = eng.run()
        got = dict(distinct=r.distinct, generated=r.generated, depth=r.depth, verdict=r.verdict, trace_len=r.trace_len, levels=list(r.levels))
        print(name, backend, got)
        assert got == {k: want[k] for k in got}, (name, backend)
        texts = eng.state_texts(0, r.distinct)
        at, views = 0, []
        for n in r.levels:   # the arena holds the states level by level
            views.append({ref.view_of_text(t) for t in texts[at:at + n]})
            at += n
        assert views == want["level_views"], (name, backend)
        if want["verdict"] == "invariant":   # the counterexample ends in the successor of the REFUSED step: rebuilt from its parent, stored nowhere
            tr = eng.trace()
            assert len(tr) == want["trace_len"] and prog.invariant(r.violated_invariant) == want["violated"]
            assert not ref.ck.ev(ref.ck.defs[want["violated"]][1], ref.state_of_text(tr[-1][1]), None, {})
    finally:
        eng.close()


@pytest.mark.parametrize("name,backend", CASES)
def test_every_model_equals_the_reference(amd, name, backend):  # noqa: F811
    check_run(amd, name, backend)


def test_wide_with_unpacked_rows_of_generated_code(amd, monkeypatch):  # noqa: F811
    monkeypatch.setenv("TLAMC_JIT_PACK", "0")

    class Handle:
        h = cfgmore.load("wide")[0].params[0]
    header = helpers.program_codegen(Handle)   # what the engine's load-time build generates under this environment
    assert "PACKED = false" in header and "view_words" in header and "run_acon" in header
    check_run(amd, "wide", "pairs")
    check_run(amd, "wide", "slots")


def test_an_evaluation_error_inside_an_action_constraint_is_a_spec_error(amd):  # noqa: F811
    prog = cfgmore.compiled("ac_error")
    eng = amd.Engine("pcal", prog.params, **KW)
    try:
        r = eng.run()
        assert (r.verdict, r.trace_len, r.distinct, r.generated) == ("spec-error", 1, 1, 2), dict(r)
    finally:
        eng.close()


def test_the_state_graph_has_exactly_the_allowed_edges(amd):  # noqa: F811
    prog, ref, want = cfgmore.load("ac_monotone")
    eng = amd.Engine("pcal", prog.params, **KW)
    try:
        r = eng.run()
        info, offsets, dst, action = eng.graph()
        texts = [t.replace("\n", " ") for t in eng.state_texts(0, r.distinct)]
        edges = {(texts[i], texts[int(d)]) for i in range(r.distinct) for d in dst[int(offsets[i]):int(offsets[i + 1])]}
        assert edges == want["edges"]
    finally:
        eng.close()


def test_coverage_counts_refused_successors_as_generated_never_distinct(amd):  # noqa: F811
    prog, ref, want = cfgmore.load("ac_monotone")
    eng = amd.Engine("pcal", prog.params, coverage=True, **KW)
    try:
        r = eng.run()
        cov = eng.coverage()
        print(cov)
        assert sum(n for _, n in cov.values()) == r.generated == want["generated"]
        assert sum(d for d, _ in cov.values()) == r.distinct == want["distinct"]
        # every step of the model is the action `s`: 18 generated successors, 12 of them refused, 5 stored states besides the initial one
        assert cov["Init"] == (1, 1) and cov["s"] == (want["distinct"] - 1, want["generated"] - 1)
        assert want["refused"] == 12 and cov["s"][1] - want["refused"] >= cov["s"][0]
    finally:
        eng.close()


def test_no_simulated_walk_takes_a_refused_step(amd, tmp_path):  # noqa: F811
    """the device's walks are the host's, slot by slot, and the host's rows of those walks are paths of the reference's graph, in which a
    refused transition is an edge that cannot be walked (tests/simgraph.py); every walk ends where all successors are refused"""
    import simgraph
    from test_gpu_simulate import same_as_host
    from test_simulate_graph import check
    prog, ref, want = cfgmore.load("ac_monotone")
    g = cfgmore.sim_graph(ref)
    for jit in (False, True):
        same_as_host(amd, "pcal", prog.params, prog.params, seed=5, n=200, depth=12, jit=jit)
    ends, _, _ = check(tmp_path, g, "pcal", prog.params, 5, 200, 12, True)
    assert ends[simgraph.END_OUT_OF_MODEL] == 200


def test_a_checkpoint_under_a_view_is_refused_without_it(amd, tmp_path):  # noqa: F811
    tla, cfg = cfgmore.texts("ghost_history")
    prog = cfgmore.load("ghost_history")[0]
    a = amd.Engine("pcal", prog.params, max_levels=5, **KW)
    a.run()
    a.checkpoint(tmp_path / "ck")
    a.close()
    plain = amd.Program(tla, cfg.replace("VIEW View\n", ""))
    b = amd.Engine("pcal", plain.params, **KW)
    try:
        with pytest.raises(amd.McError):
            b.restore(tmp_path / "ck")
    finally:
        b.close()
    c = amd.Engine("pcal", prog.params, **KW)   # ... and accepted by an engine of the same program
    try:
        c.restore(tmp_path / "ck")
        r = c.run()
        want = cfgmore.load("ghost_history")[2]
        assert (r.distinct, r.depth, r.verdict) == (want["distinct"], want["depth"], "ok")
    finally:
        c.close()


def test_mc_terminates_on_the_infinite_model_under_its_view(amd):  # noqa: F811
    want = cfgmore.load("ghost_unbounded")[2]
    p = run_mc(cfgmore.DIR / "ghost_unbounded.tla")
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert f"{want['generated']} states generated, {want['distinct']} distinct states found, 0 states left on queue." in p.stdout, p.stdout
    assert f"The depth of the complete state graph search is {want['depth']}." in p.stdout, p.stdout


def test_mc_names_termination_under_a_view_as_not_checked(amd):  # noqa: F811
    p = run_mc(cfgmore.DIR / "termination_view.tla")
    assert p.returncode == 0, (p.stdout, p.stderr)
    lines = [ln for ln in p.stdout.splitlines() if "NOT checked" in ln]
    assert len(lines) == 1 and "VIEW" in lines[0] and "Termination" in lines[0], p.stdout
