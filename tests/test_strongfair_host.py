"""Strong fairness of whole processes on the host: the front end's part (mc_program_fairness_strong beside an unchanged
mc_program_fairness, image and translation), tests/strongfair.py's reference on the models of specs_strongfair/, and liveness.h's new
functions built with g++ over the interpreter lowering (tests/_strongshim), which must give the reference's answers on every model
while five one-line mutants of them do not."""
import json

import pytest

import helpers
import livegraph
import liveprops
import strongfair

ROOT = helpers.ROOT


@pytest.fixture(scope="module")
def amd():
    import tla_rust_amd
    return tla_rust_amd


@pytest.fixture(scope="module")
def graphs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = strongfair.load(name)
        return made[name]
    yield get
    for prog, _, _ in made.values():
        prog.close()


# ------------------------------------------------------------------------------------------------ the front end
def test_fairness_masks_of_every_model(amd, graphs):
    expect = {"sem2_fair": (0b11, 0), "sem2_strong": (0, 0b11), "sem3_fair": (0b111, 0), "sem3_strong": (0, 0b111), "toggle_fair": (0b11, 0),
              "toggle_strong": (0b10, 0b01), "subcycle": (0b10, 0b01), "mixed_sf": (0b010, 0b001), "mixed_wf": (0b001, 0b010),
              "mixed_noise": (0b100, 0b001), "leftover": (0, 0b01), "ring_strong": (0b01, 0b10)}
    assert set(expect) == set(strongfair.MODELS)
    for name, (weak, strong) in expect.items():
        prog, g, _ = graphs(name)
        assert prog.strong_fairness == (weak, strong, None), name
        assert prog.fair_mask == weak | strong and prog.ninst == g.nproc            # the weak entry: unchanged
        assert (prog.live_refusal is None) == (strong == 0)
        if strong:
            assert "fair+" in prog.live_refusal


def test_refusals_that_stay(amd):
    for stem, word in strongfair.REFUSED.items():
        p = strongfair.compiled(stem)
        assert p.strong_fairness[1] == 1 and word in p.strong_fairness[2] and "fair+" in p.live_refusal
        p.close()
    for stem, word in livegraph.REFUSED.items():
        p = amd.Program((livegraph.DIR / (stem + ".tla")).read_text(), (livegraph.DIR / (stem + ".cfg")).read_text())
        weak, strong, why = p.strong_fairness
        assert word in p.live_refusal                                               # today's words, untouched
        if stem == "refused_strong":
            assert why is None and strong and not weak & strong and weak | strong == p.fair_mask
        else:
            assert why == p.live_refusal
        p.close()
    for stem in liveprops.REFUSED:                                                  # refused PROPERTIES are the properties' business
        p = liveprops.compiled(stem)
        assert p.strong_fairness == (p.fair_mask, 0, p.live_refusal)
        p.close()
    view = amd.Program((ROOT / "specs_strongfair" / "toggle_strong.tla").read_text().replace("=====", "V == <<turn>>\n====="),
                       "SPECIFICATION Spec\nPROPERTY Termination\nVIEW V\n")
    assert "VIEW" in view.strong_fairness[2] and "VIEW" in view.live_refusal
    view.close()


def test_the_keyword_changes_nothing_but_the_masks(amd):
    """`fair+` for `fair`: the same translation but for the keyword's own conjunct (SF_ for WF_), the same program image"""
    from test_liveprops_host import image_of
    for a, b in (("sem2_fair", "sem2_strong"), ("toggle_fair", "toggle_strong")):
        ta, tb = ((strongfair.DIR / (s + ".tla")).read_text() for s in (a, b))
        pa, pb = strongfair.compiled(a), strongfair.compiled(b)
        try:
            assert image_of(pa)[0] == image_of(pb)[0] and image_of(pa)[1] == image_of(pb)[1]
            assert pa.translated().replace(a, "X") != pb.translated().replace(b, "X")       # (SF_ / WF_ in Spec)
            assert pb.translated() == amd.pcal_translate(tb) and pa.translated() == amd.pcal_translate(ta)
            assert "SF_vars" in pb.translated() and "SF_vars" not in pa.translated()
        finally:
            pa.close()
            pb.close()
    # what was there before reads as before: the recorded images of the models of specs_liveprops (an existing test compares them all)
    golden = json.loads((ROOT / "tests" / "golden" / "liveprops_images.json").read_text())
    assert golden


# ------------------------------------------------------------------------------------------------ the reference on the models
@pytest.mark.parametrize("name", list(strongfair.MODELS))
def test_the_reference_gives_the_verdict_the_model_was_written_for(graphs, name):
    prog, g, checks = graphs(name)
    weak, strong, _ = prog.strong_fairness
    got = {c: strongfair.decide_model(g, prop, weak, strong) for c, prop in checks}
    assert {c: v.violated for c, v in got.items()} == strongfair.MODELS[name].expect
    if name in strongfair.ROUNDS:
        assert all(v.rounds == strongfair.ROUNDS[name] for v in got.values())
    if name.endswith("_strong") or name == "mixed_sf":      # what strong fairness buys: the same model under weak fairness is violated
        assert all(strongfair.decide_model(g, prop, weak | strong, 0).violated for _, prop in checks)
    if name == "subcycle":                                  # found in round 2; no state of the final component enables Exit
        for v in got.values():
            assert v.rounds == 2 and len(v.root) == 2 and not any(0 in g.en[i] for i in v.root)
    if name == "leftover":                                  # a one-state final component left over: the witness stutters
        for v in got.values():
            assert len(v.root) == 1 and not (g.en[min(v.root)] & {0})


def test_the_reference_equals_the_definition_on_every_small_model(graphs):
    for name in strongfair.SMALL:
        prog, g, checks = graphs(name)
        weak, strong, _ = prog.strong_fairness
        allp = (1 << g.nproc) - 1
        for w, s in ((weak, strong), (0, allp), (allp, 0), (0, 0), (strong, weak)):
            for cname, prop in checks:
                brute = strongfair.brute_force_strong(g.edges, g.en, g.nproc, len(g.init), g.bits, g.done, prop, w, s)
                if brute is None:
                    assert name.startswith("sem3") or name.startswith("mixed"), name     # (M of more than 14 states)
                    continue
                assert brute == strongfair.decide_model(g, prop, w, s).violated, (name, cname, w, s)


# ------------------------------------------------------------------------------------------------ liveness.h on the host
def check_model(name, tmp, graphs, L=None):
    import strongshim
    prog, g, checks = graphs(name)
    weak, strong, _ = prog.strong_fairness
    for cname, prop in checks:
        got = strongshim.check(prog, weak, strong, prop, tmp, L=L)
        assert got["states"] == len(g.texts)
        rank = {t: i for i, t in enumerate(got["texts"])}
        want = strongfair.decide_model(g, prop, weak, strong, rank=[rank[t] for t in g.texts])
        texts = lambda c: frozenset(g.texts[v] for v in c)   # noqa: E731
        assert not got["overrun"], f"{name} {cname}: the refinement ran into its bound, unlike the reference's"
        assert got["final"] == {texts(c) for c in want.final}, f"{name} {cname}: the final components differ from the reference's"
        assert got["components"] == len(want.final), f"{name} {cname}: the count differs from the reference's"
        assert got["ids"] == {g.texts[v]: g.texts[i] for v, i in enumerate(want.ids)}, f"{name} {cname}: the refined ids differ from the reference's"
        assert (got["rounds"], got["closed"], got["mask_states"]) == (want.rounds, want.closed, want.mask_states), f"{name} {cname}: the counts differ from the reference's"
        if prop["kind"] == strongfair.TERMINATION:
            assert got["witness"] == (g.texts[want.first_root] if want.violated else None), f"{name} {cname}: the least root differs from the reference's"
        else:
            assert got["witness"] == (g.texts[want.witness] if want.violated else None), f"{name} {cname}: the witness differs from the reference's"
            assert got["bad_starts"] == want.bad_starts, f"{name} {cname}: the bad starts differ from the reference's"
            if want.violated:
                assert [got["dist"][g.texts[v]] for v in want.path] == list(range(len(want.path) - 1, -1, -1))


@pytest.mark.parametrize("name", list(strongfair.MODELS))
def test_the_rule_on_the_host_equals_the_reference(name, tmp_path, graphs):
    check_model(name, tmp_path, graphs)


# name: (its text in liveness.h, the replacement, the model that must catch it)
MUTANTS = {
    "strong-satisfied-by-being-disabled-somewhere": ("return live_blockers(all, strong, enabled, taken) ? LIVE_BLOCKED : LIVE_FINAL;",
                                                     "return (live_blockers(all, strong, enabled, taken) & ~disabled) ? LIVE_BLOCKED : LIVE_FINAL;", "sem2_strong"),
    "blocked-component-closed-whole": ("if (cls == LIVE_BLOCKED && !live_closes_state(blockers, en)) return LIVE_ST_OPEN;",
                                       "if (cls == LIVE_BLOCKED && false) return LIVE_ST_OPEN;", "subcycle"),
    "en-from-the-open-subgraph": ("    return en;\n", "    return tk;\n", "toggle_strong"),
    "blockers-not-minus-taken": ("return strong & all & enabled & ~taken;", "return strong & all & enabled;", "mixed_wf"),
    "closed-state-kept-as-final": ("    return LIVE_ST_CLOSED;\n", "    return LIVE_ST_FINAL;\n", "leftover"),
}


def test_mutants_of_the_new_functions_are_caught(tmp_path, graphs):
    import strongshim
    import testlib
    helpers.build_shim()

    def build(name):
        return strongshim.build(csrc=testlib.mutant_tree(tmp_path, name, ("liveness.h", *MUTANTS[name][:2])), out=tmp_path / name / "_build")
    for name, so in testlib.build_mutants(MUTANTS, build).items():
        run = tmp_path / name / "run"
        run.mkdir()
        with pytest.raises(AssertionError) as e:
            check_model(MUTANTS[name][2], run, graphs, L=strongshim.load(so))
            pytest.fail(f"mutant {name} survives", pytrace=False)
        assert "the reference's" in str(e.value), (name, str(e.value)[:300])


def test_the_existing_mutant_patterns_still_occur_once():
    """the lines the existing host and device mutant tests edit are where they were: the new code calls those functions, it holds no copy"""
    live, dev = ((ROOT / "tla_rust_amd" / "csrc" / f).read_text() for f in ("liveness.h", "engine_live.h"))
    for pat in ("en_ |= 1ull << p;", "return size >= 1 && !has_done", "const uint64_t need = fair & all;", "c.done = c.done || done;",
                "return !live_in_mask(c, bits);", "if (c.kind == LIVE_EVENTUALLY) return initial;"):
        assert live.count(pat) == 1, pat
    for pat in ("live_in_start(ck, bits, v < init_states)", "scc[v] = l < r ? l : r;", "big = (unsigned)__popcll(__ballot(sz > 1))"):
        assert dev.count(pat) == 1, pat
