"""Fairness in the PlusCal front end, the reference the GPU tests rely on (tests/livegraph.py) and liveness.h itself, without a GPU:
the fairness masks and refusals of the models under specs_liveness/, pcal2tla's fairness conjuncts in the translated Spec, unchanged
text for an algorithm without `fair`, that the reference gives every model the verdict it was written to show, and — through
tests/_liveshim, a g++ build of liveness.h with a sequential SCC — that the rule the device runs gives the reference's components and
fair components on every model, while five mutants of it do not."""
import pytest

import helpers
import livegraph

ROOT = helpers.ROOT


@pytest.fixture(scope="module")
def amd():
    import tla_rust_amd
    return tla_rust_amd


def compiled(amd, stem, cfg=None):
    return amd.Program((livegraph.DIR / (stem + ".tla")).read_text(), (livegraph.DIR / ((cfg or stem) + ".cfg")).read_text())


MASKS = {"handoff": (3, 0b111), "handoff_unfair": (3, 0), "spin_flag": (2, 0b11), "spin_flag_unfair": (2, 0b01), "starve_wf": (2, 0b11),
         "self_step": (2, 0b01), "self_step_exit": (1, 0b1), "ring": (2, 0b01), "two_loops": (3, 0b100)}


@pytest.mark.parametrize("stem", list(MASKS))
def test_fairness_masks(amd, stem):
    p = compiled(amd, stem)
    try:
        assert (p.ninst, p.fair_mask) == MASKS[stem] and p.live_refusal is None
    finally:
        p.close()


@pytest.mark.parametrize("stem", list(livegraph.REFUSED))
def test_refusals_name_their_reason(amd, stem):
    p = compiled(amd, stem)
    try:
        assert p.fair_mask == 1 and p.live_refusal and livegraph.REFUSED[stem] in p.live_refusal
    finally:
        p.close()


def spec_of(text):
    at = text.index("\nSpec ==") + 1
    return text[at:text.index("\nTermination ==", at)].rstrip("\n")


def test_translated_spec_of_fair_algorithms(amd):
    want = {
        "handoff": "Spec == /\\ Init /\\ [][Next]_vars\n        /\\ \\A self \\in 0..2 : WF_vars(P(self))",
        "spin_flag": "Spec == /\\ Init /\\ [][Next]_vars\n        /\\ WF_vars(Spinner)\n        /\\ WF_vars(Setter)",
        "two_loops": "Spec == /\\ Init /\\ [][Next]_vars\n        /\\ WF_vars(Fin)",
        "refused_strong": "Spec == /\\ Init /\\ [][Next]_vars\n        /\\ SF_vars(P)",
        "handoff_unfair": "Spec == Init /\\ [][Next]_vars",
    }
    for stem, spec in want.items():
        assert spec_of(amd.pcal_translate((livegraph.DIR / (stem + ".tla")).read_text())) == spec, stem
    uni = "---- MODULE u ----\nEXTENDS Naturals\n(* --fair algorithm u\nvariables x = 0;\nbegin\n  A: x := 1;\nend algorithm *)\n====\n"
    assert spec_of(amd.pcal_translate(uni)) == "Spec == /\\ Init /\\ [][Next]_vars\n        /\\ WF_vars(Next)"
    multi = uni.replace("begin\n  A: x := 1;\n", "process P \\in 0..1\nbegin\n  A: x := 1;\nend process\n")
    assert spec_of(amd.pcal_translate(multi)) == "Spec == /\\ Init /\\ [][Next]_vars\n        /\\ \\A self \\in 0..1 : WF_vars(P(self))"
    p = amd.Program(uni, "SPECIFICATION Spec\n")
    try:
        assert (p.ninst, p.fair_mask, p.live_refusal) == (1, 1, None)
    finally:
        p.close()


def test_an_algorithm_without_fair_keeps_its_text(amd):
    text = (ROOT / "specs" / "pluscal" / "peterson.tla").read_text()   # (holds its translation: translating again must give the file back)
    assert amd.pcal_translate(text) == text and "Spec == Init /\\ [][Next]_vars\n" in text
    p = amd.Program(text, (ROOT / "specs" / "pluscal" / "peterson.cfg").read_text())
    try:
        assert (p.ninst, p.fair_mask, p.live_refusal) == (2, 0, None)
    finally:
        p.close()


def test_property_of_a_module_that_is_not_pluscal_is_still_refused(amd):
    with pytest.raises(amd.McError) as e:
        amd.spec_resolve("MCraft", (ROOT / "specs" / "MCraft.cfg").read_text() + "\nPROPERTY Termination\n")
    assert e.value.code == -9 and "PROPERTY" in str(e.value)


@pytest.mark.parametrize("name", list(livegraph.MODELS))
def test_the_reference_gives_the_verdict_the_model_was_written_for(amd, name):
    prog, g = livegraph.load(name)
    try:
        fair = g.fair_components(prog.fair_mask)
        assert bool(fair) == livegraph.MODELS[name].violated
        comps = g.components()
        assert sum(len(m) for m, _, _, _ in comps.values()) == len(g.texts)
        if name == "handoff_unfair":   # no fair process: stuttering in the first non-Done state already
            assert frozenset([g.texts[0]]) in fair
        if name == "starve_wf":        # the waiter is disabled in SOME state of the cycle, enabled in another
            cyc = next(c for c in fair if len(c) == 2)
            en = [0 in g.en[g.index[t]] for t in cyc]
            assert sorted(en) == [False, True]
        if name == "self_step":        # the unchanged step is no step: Idle is never enabled
            assert all(0 not in e for e in g.en)
        if name == "ring":
            assert max(len(c) for c in g.partition()) == 65
        if name == "two_loops":        # the cycle modulo 4 is fair; the two modulo 2 (Fin at F, Fin at F2: enabled throughout) are not
            big = sorted((c for c in g.partition() if len(c) > 1), key=len)
            assert [len(c) for c in big] == [2, 2, 4] and big[2] in fair and big[0] not in fair and big[1] not in fair
    finally:
        prog.close()


# ------------------------------------------------------------------------------------------------ liveness.h on the host
# tests/_liveshim runs liveness.h (LiveProc, live_state, live_merge, live_violates) and a sequential Tarjan over the interpreter lowering's
# graph; the components and the fair non-Done ones must be livegraph's, state text by state text.
def check_model(name, tmp, L=None):
    import liveshim
    prog, g = livegraph.load(name)
    try:
        partition, bad, counts = liveshim.check(prog, prog.fair_mask, tmp, L=L)
        assert counts["states"] == len(g.texts) and counts["procs"] == g.nproc
        assert partition == g.partition(), f"{name}: the components differ from the reference's"
        want = set(g.fair_components(prog.fair_mask))
        assert bad == want, f"{name}: {len(bad)} fair non-Done components, the reference has {len(want)}"
        assert counts["violating"] == len(want) and bool(want) == livegraph.MODELS[name].violated
    finally:
        prog.close()


@pytest.mark.parametrize("name", list(livegraph.MODELS))
def test_the_rule_on_the_host_equals_the_reference(name, tmp_path):
    check_model(name, tmp_path)


# name: (its text in liveness.h, the replacement, the model that must catch it)
MUTANTS = {
    "disabled-in-all-states": ("c.disabled = c.disabled | disabled;", "c.disabled = c.first ? disabled : (c.disabled & disabled);", "starve_wf"),
    "self-edge-taken": ("return proc >= 0 && src != dst;", "return proc >= 0;", "self_step_exit"),
    "one-state-skipped": ("return size >= 1 && !has_done", "return size > 1 && !has_done", "handoff_unfair"),
    "unfair-required": ("const uint64_t need = fair & all;", "const uint64_t need = all;", "spin_flag_unfair"),
    "done-not-excluded": ("return size >= 1 && !has_done && live_fair", "return size >= 1 && live_fair", "handoff"),
}


def test_mutants_of_the_rule_are_caught(tmp_path):
    import liveshim
    import testlib
    helpers.build_shim()

    def build(name):
        return liveshim.build_liveshim(csrc=testlib.mutant_tree(tmp_path, name, ("liveness.h", *MUTANTS[name][:2])), out=tmp_path / name / "_build")
    for name, so in testlib.build_mutants(MUTANTS, build).items():
        run = tmp_path / name / "run"
        run.mkdir()
        with pytest.raises(AssertionError) as e:
            check_model(MUTANTS[name][2], run, L=liveshim.load(so))
            pytest.fail(f"mutant {name} survives", pytrace=False)
        assert "fair non-Done components" in str(e.value), (name, str(e.value)[:300])
