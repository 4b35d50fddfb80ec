"""The front end of the checks label by label, without a GPU: the models of specs_labelfair/ show what their
comments say under the reference of tests/labelfair.py; the translation prints pcal2tla's conjuncts for `+` / `-` labels and nothing
else changes; Program.fairness_units holds the units and conjuncts the reference finds edge by edge; the refusals that stay; the
patterns the existing mutant tests edit still occur once."""
import glob

import pytest

import helpers
import labelfair
import livegraph
import liveprops
import strongfair

ROOT = helpers.ROOT


@pytest.fixture(scope="module")
def amd():
    helpers.build_shim()
    import tla_rust_amd
    return tla_rust_amd


_refs = {}


def reference(name):
    if name not in _refs:
        _refs[name] = labelfair.load(name)
    return _refs[name]


@pytest.mark.parametrize("name", list(labelfair.MODELS))
def test_the_models_show_what_they_were_written_to_show(amd, name):
    prog, g, checks = reference(name)
    assert {c for c, _ in checks} == set(labelfair.MODELS[name].expect)
    for cname, prop in checks:
        assert labelfair.decide_model(g, prop).violated == labelfair.MODELS[name].expect[cname], cname


def test_the_twins_differ_in_the_modifier_alone(amd):
    """each pair answers differently — the label modifier decides —, and a `+` under `fair+` changes no answer"""
    for a, b in (("lock_plus", "lock_weak"), ("spin_minus", "spin_fair")):
        (_, ga, ca), (_, gb, cb) = reference(a), reference(b)
        for (na, pa), (nb, pb) in zip(ca, cb):
            assert na == nb and labelfair.decide_model(ga, pa).violated != labelfair.decide_model(gb, pb).violated
    for a, b in (("fairplus_plus", "fairplus_plain"),):
        (_, ga, ca), (_, gb, cb) = reference(a), reference(b)
        assert [labelfair.decide_model(ga, p).violated for _, p in ca] == [labelfair.decide_model(gb, p).violated for _, p in cb]


@pytest.mark.parametrize("name", list(labelfair.EXPECT))
def test_the_translation_prints_the_conjuncts(amd, name):
    prog = labelfair.compiled(name)
    try:
        spec, per_instance = labelfair.EXPECT[name]
        assert labelfair.spec_conjuncts(prog.translated(label_fair=True)) == spec
        fu, texts, why = prog.fairness_units
        assert why is None and texts == per_instance and fu.nconj == len(texts)
        assert fu.weak_mask == sum(1 << k for k, t in enumerate(texts) if t.startswith("WF_"))
        assert fu.strong_mask == sum(1 << k for k, t in enumerate(texts) if t.startswith("SF_"))
        # outside Spec the two translations are one text
        a, b = prog.translated(), prog.translated(label_fair=True)
        cut = lambda t: t[:t.index("\nSpec ==")] + t[t.index("\nTermination =="):]   # noqa: E731
        assert cut(a) == cut(b)
    finally:
        prog.close()


def test_the_units_table(amd):
    """units 0 .. ninst - 1 are the instances' own; a `+` label's unit sits in two conjuncts, a `-` label's and an unfair process's in none"""
    def table(name):
        prog = labelfair.compiled(name)
        try:
            fu, texts, _ = prog.fairness_units
            return prog.ninst, [fu.of_unit[u] for u in range(fu.nunits)], texts
        finally:
            prog.close()
    ninst, of_unit, texts = table("lock_plus")
    assert ninst == 2 and of_unit == [0b0001, 0b0100, 0b0011, 0b1100]
    ninst, of_unit, texts = table("spin_minus")
    assert of_unit == [0b01, 0b10, 0]
    ninst, of_unit, texts = table("unfair_plus")
    assert of_unit == [0, 0b1] and texts == ["WF_vars(Toggler)"]          # a `+` in an unfair process is not honoured
    ninst, of_unit, texts = table("fairplus_plus")
    assert of_unit == [0b01, 0b10]                                        # a `+` under fair+ adds nothing
    ninst, of_unit, texts = table("uni_minus")
    assert ninst == 1 and of_unit == [0b1, 0]


def test_a_program_without_these_forms_keeps_its_translation_and_gets_the_identity(amd):
    """every module of the repository's model folders that compiles: without `+` / `-` labels in a fair process the translation asked
    for label by label is the default one; without `fair+` too, the units are the instances and the masks mc_program_fairness's"""
    seen = 0
    for f in sorted(glob.glob(str(ROOT / "specs_liveness" / "*.tla")) + glob.glob(str(ROOT / "specs_strongfair" / "*.tla")) +
                    glob.glob(str(ROOT / "specs_liveprops" / "*.tla"))):
        cfg = f[:-4] + ".cfg"
        try:
            prog = amd.Program(open(f).read(), open(cfg).read())
        except (amd.McError, OSError):
            continue
        try:
            weak, strong, why_strong = prog.strong_fairness
            fu, texts, why = prog.fairness_units
            if why_strong is None:
                seen += 1
                assert prog.translated(label_fair=True) == prog.translated(), f
                assert why is None and fu.nunits == prog.ninst
                fair = [k for k in range(prog.ninst) if (weak | strong) >> k & 1]
                assert [fu.of_unit[u] for u in range(fu.nunits)] == [1 << fair.index(u) if u in fair else 0 for u in range(prog.ninst)], f
                assert fu.strong_mask == sum(1 << fair.index(k) for k in fair if strong >> k & 1)
                assert fu.weak_mask == sum(1 << fair.index(k) for k in fair if weak >> k & 1)
            elif "VIEW" in why_strong:
                assert why == why_strong, f
        finally:
            prog.close()
    assert seen >= 25


def test_the_process_level_answers_are_what_they_were(amd):
    """mc_program_fairness / mc_program_fairness_strong keep their answers for the new models; the default translation keeps one
    conjunct per fair process"""
    for name in ("lock_plus", "spin_minus", "toggle_plus", "two_labels_minus"):
        prog = labelfair.compiled(name)
        try:
            assert "modifier" in prog.live_refusal and "modifier" in prog.strong_fairness[2]
            assert all("notin" not in c and not c.startswith("SF_") for c in labelfair.spec_conjuncts(prog.translated()))
        finally:
            prog.close()
    prog = labelfair.compiled("unfair_plus")
    assert prog.live_refusal is None and prog.strong_fairness[2] is None and prog.fairness_units[2] is None
    prog.close()


def test_refusals(amd):
    view = amd.Program((labelfair.DIR / "toggle_plus.tla").read_text().replace("=====", "V == <<turn>>\n====="), "SPECIFICATION Spec\nPROPERTY Termination\nVIEW V\n")
    assert "VIEW" in view.fairness_units[2]
    view.close()
    proc = amd.Program((livegraph.DIR / "refused_procedure.tla").read_text(), (livegraph.DIR / "refused_procedure.cfg").read_text())
    assert proc.fairness_units[2] is None and "procedures" in proc.live_refusal and "procedures" in proc.strong_fairness[2]   # (checked label by label alone)
    proc.close()
    many = """---- MODULE many ----
EXTENDS Naturals
(* --algorithm many
variables x = 0;
fair process P \\in 0..%d
begin
  a:%s x := 1;
end process
end algorithm *)
====
"""
    conj = amd.Program(many % (32, "+"), "SPECIFICATION Spec\nPROPERTY Termination\n")       # 33 WF + 33 SF conjuncts
    assert "66 fairness conjuncts (at most 64)" in conj.fairness_units[2]
    conj.close()
    units = amd.Program(many.replace("end process", "  b: x := 2;\nend process") % (63, "-"),
                        "SPECIFICATION Spec\nPROPERTY Termination\n")                      # 64 instances, each its own unit and one of `-` labels
    assert "128 fairness units (at most 127)" in units.fairness_units[2]
    units.close()


# ---------------------------------------------------------------------------------------------------------------- the rule built with g++
def check_shim(name, tmp, L=None, shim=None):
    """tests/_unitshim on a model — the front end's table, the unit of every edge, the rule — against tests/labelfair.py, which has
    the conjunct edges from the oracle's evaluation of every conjunct's own text: the two sides share the program text alone"""
    import unitshim
    prog, g, checks = reference(name)
    m = labelfair.MODELS[name]
    sp = unitshim.Program((labelfair.DIR / m.tla).read_text(), (labelfair.DIR / m.cfg).read_text(), L=L)
    try:
        assert sp.refusal is None and sp.conjuncts == labelfair.EXPECT[name][1], "the shim's conjuncts are not the expected texts"
        for cname, prop in checks:
            got = sp.check(prop, tmp)
            want = labelfair.decide_model(g, prop)
            assert sorted(got["texts"]) == sorted(g.texts)
            assert got["violated"] == want.violated == m.expect[cname], f"{cname}: the shim's verdict is not the reference's"
            assert got["final"] == {frozenset(g.texts[v] for v in c) for c in want.final}, f"{cname}: the shim's final components are not the reference's"
            assert (got["rounds"], got["closed"], got["overrun"]) == (want.rounds, want.closed, 0), f"{cname}: rounds / closed states are not the reference's"
        # the conjuncts of every edge's unit against the reference's membership: the edges i -> j together have exactly the conjuncts
        # that, by their own TLA+ text, have a step i -> j
        by_pair = {}
        for a, b, u, ks in got["edges"]:
            if u < 0:
                assert a == b and g.done[g.index[a]], "a unit -1 on an edge that is not the terminating disjunct's"
                continue
            by_pair.setdefault((a, b), set()).update(ks)
        for (a, b), ks in by_pair.items():
            assert ks == g.members(g.index[a], g.index[b]), f"the conjuncts of the edges {a} -> {b} are not the reference's"
    finally:
        sp.close()


@pytest.mark.parametrize("name", list(labelfair.MODELS))
def test_the_rule_on_the_host_equals_the_reference(amd, name, tmp_path):
    check_shim(name, tmp_path)


# name: (the file, its text, the replacement, the model that must catch it) — one-line edits of the new host code
MUTANTS = {
    "minus-label-counted-into-the-wf-conjunct": ("pcal_compile.cpp", " && std::find(g.minus.begin(), g.minus.end(), l.label) == g.minus.end())", ")", "spin_minus"),
    "plus-label-removed-from-its-process-conjunct": ("pcal.cpp", "            g.labels.push_back(l.label);", "            if (l.mod != '+' || fair != 1) g.labels.push_back(l.label);", "toggle_plus"),
    "procedure-labels-given-the-callers-unit": ("pcal_compile.cpp", ': l.section + "|" + cls;', ': std::string() + "|" + cls;', "treiber_procs"),
    "plus-honoured-in-an-unfair-process": ("pcal.cpp", "if (l.mod == '+' && fair == 1 && std::find(plus.begin()", "if (l.mod == '+' && fair != 2 && std::find(plus.begin()", "unfair_plus"),
    "label-taken-from-the-destination-state": ("unitshim.cpp", "live_edge_unit<S>(prm, src_row, utab, slot)", "live_edge_unit<S>(prm, dst_row, utab, slot)", "two_labels_minus"),
}


def test_mutants_of_the_new_host_code_are_caught(amd, tmp_path):
    import testlib
    import unitshim

    def build(name):
        d = testlib.mutant_tree(tmp_path, name, MUTANTS[name][:3], also=(*testlib.FRONT_END, unitshim.SHIM_DIR / "unitshim.cpp"))
        return unitshim.build(csrc=d, out=tmp_path / name / "build", shim_src=d / "unitshim.cpp" if MUTANTS[name][0] == "unitshim.cpp" else None)
    libs = testlib.build_mutants(MUTANTS, build)
    for name in libs:
        (tmp_path / name / "run").mkdir()
        with pytest.raises(AssertionError) as e:
            check_shim(MUTANTS[name][3], tmp_path / name / "run", L=unitshim.load(libs[name]))
        assert "the reference's" in str(e.value) or "expected texts" in str(e.value), (name, str(e.value)[:300])
        print(name, "caught by", MUTANTS[name][3], ":", str(e.value)[:120])


def test_the_existing_mutant_patterns_still_occur_once():
    """the lines the existing host and device mutant tests edit are where they were: the new code calls those functions or stands beside
    them, it holds no copy"""
    live, dev = ((ROOT / "tla_rust_amd" / "csrc" / f).read_text() for f in ("liveness.h", "engine_live.h"))
    for pat in ("en_ |= 1ull << p;", "return size >= 1 && !has_done", "const uint64_t need = fair & all;", "c.done = c.done || done;",
                "return !live_in_mask(c, bits);", "if (c.kind == LIVE_EVENTUALLY) return initial;", "    return en;\n", "    return LIVE_ST_CLOSED;\n",
                "return strong & all & enabled & ~taken;", "return proc >= 0 && src != dst;"):
        assert live.count(pat) == 1, pat
    for pat in ("live_in_start(ck, bits, v < init_states)", "scc[v] = l < r ? l : r;", "big = (unsigned)__popcll(__ballot(sz > 1))",
                "live_blockers(all, strong, en_c, tk), en);", "const uint64_t tk = taken[c], en_c = enabled[c], o = offsets[v];",
                "const bool bad = root && live_violates_strong("):
        assert dev.count(pat) == 1, pat
