"""The safety parts of a cfg PROPERTY on compiled PlusCal programs, without a GPU: the front end reads `[][A]_v`, `[]P`
and initial predicates out of the models of specs_actprop/ and refuses what it must; the compiled program — on the host build of the
interpreter and as generated code — agrees with the reference of tests/actprop.py and with the product's own host evaluator; a cfg
without such a property compiles to what it did; -continue's rules hold for a pair that breaks a property of a step; and three
one-line mutants of the new code are each caught by the model written for it."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest

import actprop
import cfgmore
import helpers
import testlib

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

COUNTS = ("verdict", "trace_len", "distinct", "generated", "depth", "levels")
ST_ENABLED, ST_OUT_OF_MODEL, ST_INVARIANT, ST_SELFLOOP = 1, 2, 8, 64   # mc_common.h


@pytest.fixture(scope="module")
def amd():
    import tla_rust_amd as amd
    amd.lib()
    return amd


def name_of(amd, prog, index):
    L = amd.binding.lib()
    L.mc_invariant_name.restype = C.c_char_p
    L.mc_invariant_name.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_int]
    return L.mc_invariant_name(C.byref(helpers.spec_desc("pcal", prog.params)), index).decode() if index >= 0 else None


def test_the_status_bits_are_the_headers():
    text = (ROOT / "tla_rust_amd" / "csrc" / "mc_common.h").read_text()
    for name, v in (("ST_ENABLED", ST_ENABLED), ("ST_INVARIANT", ST_INVARIANT), ("ST_OUT_OF_MODEL", ST_OUT_OF_MODEL), ("ST_SELFLOOP", ST_SELFLOOP)):
        assert f"{name} = {v}u" in text, name


@pytest.mark.parametrize("name", list(actprop.MODELS))
def test_the_reference_shows_what_the_model_was_written_for(name):
    m, (prog, ref, r) = actprop.MODELS[name], actprop.load(name)
    assert (r["verdict"], r["violated"], r["trace_len"]) == (m.verdict, m.violated, m.trace_len)
    assert m.distinct is None or r["distinct"] == m.distinct
    assert ref.props, "the cfg names no safety part"


def test_what_each_model_shows():
    load = actprop.load
    # ap_monotone_ok: counts and levels are those of the search without the PROPERTY
    prog, _, r = load("ap_monotone_ok")
    plain = actprop.Reference(prog, *actprop.texts("ap_monotone_ok_plain")).run()
    assert all(r[k] == plain[k] for k in COUNTS + ("level_lines",))
    # ap_seen: the violating step ends in the initial state — no state of the behaviour's last level is new
    _, _, r = load("ap_seen")
    assert r["distinct"] == 3 and r["last_step"][1] == r["level_lines"][0][0] and r["levels"] == [1, 1, 1]
    # ap_subscript: the step that breaks the tuple's property leaves x alone
    _, ref, r = load("ap_subscript_tuple")
    assert "x = 0" in r["last_step"][0] and "x = 0" in r["last_step"][1] and load("ap_subscript")[2]["verdict"] == "ok"
    # ap_done: the terminating disjunct is generated (one successor more than states that step) and is no violation
    _, _, r = load("ap_done")
    assert r["generated"] == r["distinct"] + 1
    # ap_spec: the fairness conjunct is the liveness part; the other cfgs break the step formula and the initial predicate
    assert [c for _, c in load("ap_spec")[1].live] == ["WF_hv(HNext)"]
    assert load("ap_spec_badstep")[2]["last_step"] is not None and load("ap_spec_badinit")[2]["last_step"] is None
    # ap_always: what INVARIANT x <= 3 gives
    prog, _, r = load("ap_always")
    inv = actprop.Reference(prog, *actprop.texts("ap_always_inv")).run()
    assert all(r[k] == inv[k] for k in COUNTS + ("level_lines",)) and (r["violated"], inv["violated"]) == ("Small", "Le3")
    # ap_refused_step: the violating steps are exactly refused ones, and none of them is stored
    prog, ref, r = load("ap_refused_step")
    assert r["step_violations"]["Mono"] and all("x = 1" in n for _, n in r["step_violations"]["Mono"]) and not any("x = 1" in s for s in r["level_lines"][1])
    # ap_mixed: one conjunct for the search, one for the state graph
    assert [c for _, c in load("ap_mixed")[1].live] == ["((x = 0) ~> (x = 2))"] and len(load("ap_mixed")[1].props) == 1
    # ap_two: all three are violated out of the initial state; the successor that breaks Inv breaks KeepX too
    _, _, r = load("ap_two")
    assert set(r["step_violations"]) == {"KeepX", "KeepY"} and set(r["state_violations"]) == {"Inv"}
    assert {n for _, n in r["step_violations"]["KeepX"]} == r["state_violations"]["Inv"]


def test_programs_list_their_action_properties(amd):
    expect = {
        "ap_monotone": [("Mono", "step", 0, "[ ] [ x ' >= x ] _x")],
        "ap_subscript_tuple": [("IncXY", "step", 0, "[ ] [ x ' = x + 1 ] _ << x , y >>")],
        "ap_spec": [("HSpec", "step", 0, "[ ] [ HNext ] _hv"), ("HSpec", "init", 1, "HInit")],
        "ap_spec_badinit": [("HSpecOne", "step", 0, "[ ] [ HNext ] _hv"), ("HSpecOne", "init", 1, "x = 1")],
        "ap_always": [("Small", "always", 0, "[ ] ( x <= 3 )")],
        "ap_mixed": [("Both", "step", 0, "[ ] [ x ' >= x ] _x")],
        "ap_two": [("KeepX", "step", 1, "[ ] [ x ' <= 1 ] _x"), ("KeepY", "step", 2, "[ ] [ y ' = y ] _y")],   # (index 0 is the INVARIANT)
    }
    for name, want in expect.items():
        prog = actprop.load(name)[0]
        assert [(a.origin, a.kind, a.index, a.text) for a in prog.action_properties] == want, name
        for a in prog.action_properties:
            assert name_of(amd, prog, a.index) == a.origin
    assert [a.origin for a in actprop.load("ap_kinds")[0].action_properties] == ["KPc", "KLocal", "KField", "KLen", "KSet"]
    two = actprop.load("ap_two")[0]
    assert name_of(amd, two, 0) == "Inv" and name_of(amd, two, 3) == "?"
    # past the last, and without a program
    L = amd.binding.lib()
    ap = amd.binding.ActionProperty()
    assert L.mc_program_action_property(two._h, 2, C.byref(ap)) == -1 and L.mc_program_action_property(None, 0, C.byref(ap)) == -1   # MC_EBADCFG
    # the liveness side of the same names: the safety-only ones are refused THERE with the word, the mixed one is a check, the fairness conjunct is named
    assert all(lp.refused and "safety" in lp.reason for lp in two.live_properties)
    assert [(lp.origin, lp.refused, lp.kind) for lp in actprop.load("ap_mixed")[0].live_properties] == [("Both", False, 0)]
    lp, = actprop.load("ap_spec")[0].live_properties
    assert lp.refused and "WF_hv ( HNext )" in lp.reason and "WF_" in lp.reason


def test_a_state_predicate_or_a_fairness_formula_alone_stays_what_it_was(amd):
    """an initial predicate and a WF_ conjunct count beside a `[][A]_v` only: without one the PROPERTY is refused as before, whole"""
    tla = actprop.texts("ap_spec")[0]
    for body, word in (("<>(x = 2) /\\ WF_hv(HNext)", "WF_"), ("HInit /\\ <>(x = 2)", "not one of")):
        p = amd.Program(tla.replace("HSpecOne == (x = 1) /\\ [][HNext]_hv", "HSpecOne == " + body), "SPECIFICATION Spec\nPROPERTY HSpecOne\n")
        assert p.action_properties == [] and [(lp.refused, word in lp.reason) for lp in p.live_properties] == [(True, True)]
        p.close()


@pytest.mark.parametrize("name", list(actprop.REFUSED))
def test_refusals_name_their_reason(amd, name):
    with pytest.raises(amd.McError) as e:
        amd.Program(*actprop.texts(name))
    assert actprop.REFUSED[name] in str(e.value), str(e.value)


def test_more_refusals(amd):
    tla = actprop.texts("ap_two")[0]
    for body, word in (("[][a]_x", "names `a`"), ("[][x' >= x]_Inv", "subscript"),
                       ("[][x' >= x]_x /\\ <<x' > x>>_x", "<<A>>_v"), ("[][<>(x = 1)]_x", "temporal")):
        with pytest.raises(amd.McError) as e:
            amd.Program(tla.replace("KeepY == [][y' = y]_y", "KeepY == " + body), "SPECIFICATION Spec\nPROPERTY KeepY\n")
        assert word in str(e.value), (body, str(e.value))
    # the index of a violation has 5 bits: invariants + properties above 32 cannot be told apart (8 per kind is the nearer limit)
    many = "".join(f"Q{k} == [](x >= 0)\n" for k in range(9))
    with pytest.raises(amd.McError) as e:
        amd.Program(tla.replace("Inv == x < 2", many + "Inv == x < 2"), "SPECIFICATION Spec\nPROPERTY " + " ".join(f"Q{k}" for k in range(9)) + "\n")
    assert "at most 8 invariants" in str(e.value)


def check_model(name, tmp_path, search=None, prog=None):
    """a host build of the interpreter (`search`: a mutant's) against the reference: verdict, violated name, counts, the behaviour's length,
    its last step breaking A, and the states per level"""
    prog0, ref, want = actprop.load(name)
    prog = prog or prog0
    got = (search or actprop.host_search)(prog)
    print(name, {k: got[k] for k in COUNTS}, got["violated"], {k: want[k] for k in COUNTS}, want["violated"])
    assert {k: got[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, ("counts differ from the reference", name)
    names = [a.origin for a in prog0.action_properties]
    violated = None if got["violated"] < 0 else next((a.origin for a in prog0.action_properties if a.index == got["violated"]), None) or ref.invariants[got["violated"]]
    assert violated == want["violated"], name
    if want["last_step"]:
        assert (got["before"], got["after"]) == want["last_step"] and ref.breaks(want["violated"], got["before"], got["after"]), name
    elif want["verdict"] == "invariant" and want["violated"] in names and want["trace_len"] > 1:   # a `[]P`: the last state breaks P
        assert got["after"] in want["state_violations"][want["violated"]]
    return got


@pytest.mark.parametrize("name", list(actprop.MODELS))
def test_the_interpreter_on_the_host_equals_the_reference(name, tmp_path):
    check_model(name, tmp_path)
    prog, ref, want = actprop.load(name)
    dump = tmp_path / "d"
    got = helpers.shim_run("pcal", prog.params, dump=str(dump))   # tests/_shim's search: the same counts, and the states per level
    assert (got["verdict"], got["trace_len"], got["distinct"], got["generated"], got["levels"], got["fp_mismatch"]) == \
           (want["verdict"], want["trace_len"], want["distinct"], want["generated"], want["levels"], 0)
    assert actprop.level_lines_of_dump(dump) == want["level_lines"]


class _Handle:   # what helpers.program_codegen needs of a program
    def __init__(self, prog):
        self.h = prog.params[0]


@pytest.mark.parametrize("name,pack", [("ap_seen", "1"), ("ap_kinds_bad", "1"), ("ap_kinds", "0"), ("ap_spec_badinit", "1"), ("ap_two", "0"), ("ap_refused_step", "1")])
def test_generated_code_equals_the_interpreter(name, pack, monkeypatch):
    """tests/_cfgmore/harness_cfg.cpp's route: generated code against SpecVmCfg on every reachable state and slot — statuses (the
    property's index among them), rows, fingerprints"""
    monkeypatch.setenv("TLAMC_JIT_PACK", pack)
    prog, _, want = actprop.load(name)
    text = helpers.program_codegen(_Handle(prog))
    assert ("NAPROP" in text) == ("run_aprop" in text) == any(a.kind != "always" for a in prog.action_properties)
    g = cfgmore.gen_check(prog)
    print(name, pack, g)
    assert g["mismatches"] == 0 and g["pairs_checked"] > 0, g
    if want["verdict"] == "ok":
        assert (g["distinct"], g["generated"], g["depth"]) == (want["distinct"], want["generated"], want["depth"])


def test_the_host_evaluator_gives_the_same_verdict(tmp_path):
    """the product's own host evaluator (tlaeval.cpp compile_property) on the translated module and the same cfg"""
    for name in ("ap_monotone", "ap_spec", "ap_spec_badinit", "ap_always", "ap_subscript"):
        prog, _, want = actprop.load(name)
        module = re.search(r"MODULE (\w+)", prog.translated()).group(1)   # (a module is read from the file of its name)
        (tmp_path / f"{module}.tla").write_text(prog.translated())
        r = helpers.tlaeval_run(tmp_path / f"{module}.tla", actprop.DIR / f"{name}.cfg")
        assert r["rc"] == 0, (name, r)
        assert (helpers.VERDICTS[r["verdict"]], r["distinct"], r["generated"], r["depth"]) == (want["verdict"], want["distinct"], want["generated"], want["depth"]), (name, r)


def test_a_cfg_without_a_property_compiles_to_what_it_did(amd):
    """tests/test_cfgmore_host.py pins image, VmParams and generated header of the older cfgs against tests/golden/liveprops_images.json;
    here: a program WITH a `[][A]_v` keeps the image of the program without it as a prefix (the length word apart), its table behind
    the image grows by one entry per property, and only its generated header knows the members"""
    import test_liveprops_host as t
    from array import array
    tla = actprop.texts("ap_monotone")[0]
    with_, without = actprop.load("ap_monotone")[0], amd.Program(tla, actprop.texts("ap_monotone_plain")[1])
    (a, fa), (b, fb) = t.image_of(with_), t.image_of(without)
    wa, wb = list(array("i", a)), list(array("i", b))
    n_hdr = 24
    code_len = next(i for i in range(n_hdr) if wa[i] != wb[i])   # the only header word that differs: the length
    assert (wa[code_len], wb[code_len]) == (len(wa), len(wb)) and wa[:code_len] + wa[code_len + 1:len(wb)] == wb[:code_len] + wb[code_len + 1:]
    h_with, h_without = t.header_of(amd, with_), t.header_of(amd, without)
    assert "run_aprop" in h_with and "NAPROP = 1, NINITP = 0" in h_with and "aprop" not in h_without and "NINITP" not in h_without
    # (the same module with the PROPERTY named twice, or beside Termination, is the same program)
    twice = amd.Program(tla, "SPECIFICATION Spec\nPROPERTY Mono Termination Mono\n")
    assert t.image_of(twice)[0] == a
    for p in (without, twice):
        p.close()


def test_the_continue_rules_with_a_property_of_a_step(amd):
    """violations.h with the model's number of invariants: a pair whose index lies behind them is fatal — new or not, inside the model or
    not — and no stored state is listed under such an index; below it everything is as it was"""
    L = actprop.actshim_lib()

    def pair(st, ninv):
        out = [C.c_uint() for _ in range(3)]
        L.actshim_pair(st, ninv, *[C.byref(x) for x in out])
        return tuple(x.value for x in out)
    NONE, OUTSIDE, FATAL = 0, 1, 2
    inv = lambda k: ST_ENABLED | ST_INVARIANT | k << 8
    assert pair(inv(1), 2) == (NONE, 1, 1) and pair(inv(1) | ST_OUT_OF_MODEL, 2) == (OUTSIDE, 1, 1)      # an invariant: the stored pass counts it
    for extra in (0, ST_OUT_OF_MODEL, ST_SELFLOOP):
        assert pair(inv(2) | extra, 2) == (FATAL, actprop.BIN_FATAL, 2)                                   # a property of a step
    assert pair(ST_ENABLED, 2)[0] == NONE and pair(inv(2), 3)[0] == NONE
    assert L.actshim_stored_bin(inv(1), 2) == 1 and L.actshim_stored_bin(inv(2), 2) == -1 and L.actshim_stored_bin(inv(2) | ST_OUT_OF_MODEL, 3) == -1
    # ap_two under -continue: the search ends at the end of level 1; the invariant's row is the reference's (one stored state), the
    # property's pair is fatal — KeepY's, the only step that breaks a property and no invariant
    prog, ref, want = actprop.load("ap_two")
    got = actprop.host_search(prog, cont=True)
    assert got["fatal"] and name_of(amd, prog, got["fatal_inv"]) == "KeepY" and got["fatal_pairs"] == 1 and got["depth"] == 2
    assert got["states"][0] == len(want["state_violations"]["Inv"]) == 1 and sum(got["states"]) == 1 and sum(got["outside"]) == 0
    # ap_refused_step: the violating steps are outside the model (refused) and fatal all the same
    prog, ref, want = actprop.load("ap_refused_step")
    got = actprop.host_search(prog, cont=True)
    assert got["fatal"] and got["fatal_pairs"] == len(want["step_violations"]["Mono"]) and sum(got["states"]) == 0


# name: (file, its text, the replacement, the model that must catch it)
MUTANTS = {
    "subscript-ignored": ("pcal.cpp", "if (!unchanged.empty()) {   // ( \\A .. : ( A ) ) \\/ UNCHANGED v", "if (false) {", "ap_subscript"),
    "cur-and-succ-swapped": ("spec_vm_cfg.h", "const_cast<int32_t *>(cur), res, aux, succ);", "const_cast<int32_t *>(succ), res, aux, cur);", "ap_seen"),
    "refused-step-not-checked": ("spec_vm_cfg.h", "if (!(st & ST_SPECERR)) st |= ap;", "if (!(st & (ST_SPECERR | ST_OUT_OF_MODEL))) st |= ap;", "ap_refused_step"),
    "defined-subscript-dropped": ("pcal_compile.cpp", "if (x->k == Expr::TUPLE) { next.insert(next.end(), x->a.begin(), x->a.end()); changed = true; }",
                                "if (x->k == Expr::TUPLE) { changed = true; }", "ap_spec_badstep"),   # (`hv == <<x, y>>`: the subscript through a definition)
}


def test_mutants_of_the_new_code_are_caught(tmp_path):
    """each mutant is a whole front end + interpreter of its own (tests/_actshim's library with the front end compiled in, built from a
    copy of the sources with one edit); the model is compiled BY the mutant and searched by it"""
    def build(name):
        d = testlib.mutant_tree(tmp_path, name, MUTANTS[name][:3], also=testlib.FRONT_END)
        return actprop.build_actshim(csrc=d, out=tmp_path / name / "act", own_front_end=True)
    for name, so in testlib.build_mutants(MUTANTS, build).items():
        model = MUTANTS[name][3]
        L = actprop.actshim_lib(so)
        L.actshim_compile.restype = C.c_void_p
        L.actshim_compile.argtypes = [C.c_char_p] * 4
        tla, cfg = actprop.texts(model)
        c = cfgmore.read_cfg(cfg)
        h = L.actshim_compile(tla.encode(), " ".join(c["PROPERTY"]).encode(), " ".join(c["INVARIANT"]).encode(), " ".join(c["ACTION_CONSTRAINT"]).encode())
        if not h:   # (a mutant that no longer compiles the model is caught too)
            continue

        class Prog:
            params = [h]
        with pytest.raises(AssertionError):
            check_model(model, tmp_path, search=lambda p, L=L: actprop.host_search(p, lib=L), prog=Prog)
            pytest.fail(f"mutant {name} survives", pytrace=False)
