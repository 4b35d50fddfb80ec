"""What -continue collects, on the host (tla_rust_amd/csrc/violations.h through tests/_contshim, no GPU), against the references of
tests/contshim.py: per entry of the summary — every invariant index of the model, deadlock, the fatal error — the distinct stored
states, the successors outside the model and the level of the first violator must be the reference's, the search must reach exactly
the reference's states (dump against dump), and the first stored violator the host names must break that invariant in the reference.

Mutants of violations.h (test_mutants_are_killed builds each and asserts that its model fails) and what kills each:
  parentless-skipped     a state without a parent is not evaluated      init_breaks: Positive loses its level-1 violator
  outside-is-state       an outside successor counts as a stored state  outside_only: Under gets states, loses outside
  fatal-not-separated    every flagged pair ends the search             pcal_intro: the run ends at the first MoneyInvariant level
"""
import subprocess

import pytest

import contshim
import helpers
import testlib

ROOT = helpers.ROOT
SSI_NAMES = ["WellFormed", "CorrectnessOfHoldingXLocks", "CorrectnessOfWaitingForXLock", "CorrectReadView", "FirstCommitterWins", "CahillOK",
             "BernsteinOK", "(expected-to-be-violated predicate)"]
# name: (spec, params, oracle params, invariant names, deadlock)
HAND = {
    "ssi2x2": ("ssi", [2, 2, 127, 2], [2, 2, 127, 2], SSI_NAMES, True),
    "ssi2x1": ("ssi", [2, 1, 127, 1], [2, 1, 127, 1], SSI_NAMES, True),
    "voting": ("paxos", [1, 3, 2, 2, 1, 0, 1], [1, 3, 2, 2, 1, 0, 1], ["Inv"], True),   # (the PROPERTY is no row: violations.h ViolModel<SpecPaxos>)
    "pcal_intro": ("pcal_intro", [1, 1, 20, 2], [1, 1, 20, 2], ["MoneyInvariant"], True),
}
PCAL = ["many_wrongs", "init_breaks", "outside_only"]


def compare(tag, r, ref, host_dump, ref_texts_by_level):
    want = ref.entries()
    print(tag, "host", r["entries"], "reference", want)
    assert len(r["entries"]) == len(want), (tag, [e["kind"] for e in r["entries"]], [e["kind"] for e in want])
    for got, w in zip(r["entries"], want):
        for key in ("kind", "states", "outside", "first_level"):
            assert got[key] == w[key], f"{tag}: {w['name']}.{key} = {got[key]}, the reference has {w[key]}"
    assert (r["distinct"], r["generated"], r["depth"], r["levels"]) == (ref.distinct, ref.generated, ref.depth, ref.levels), tag
    assert helpers.read_dump(host_dump) == ref_texts_by_level, tag
    lines = [ln.rstrip("\n").split(" ", 1)[1] for ln in open(host_dump)]
    for got, w in zip(r["entries"], want):
        if w["kind"] == "invariant" and w["states"]:
            assert ref.breaks(lines[got["first_state"]], w["invariant"]), (tag, w["name"], lines[got["first_state"]])
        if w["kind"] == "deadlock" and w["states"]:
            assert ref.dead[ref.index[lines[got["first_state"]]]], (tag, lines[got["first_state"]])


def kept_by_level(ref):
    by = {}
    for k in ref.kept:
        by.setdefault(ref.level[k], []).append(ref.text[k])
    return {lv: sorted(v) for lv, v in by.items()}


def check_hand(tmp, name, L=None):
    spec, params, oparams, names, deadlock = HAND[name]
    ref = contshim.oracle_reference(spec, oparams, names, tmp, deadlock=deadlock)
    r = contshim.search(spec, params, deadlock=deadlock, dump=tmp / "host.txt", L=L)
    # (the hand lowerings list every invariant index they know; the reference has their names)
    compare(name, r, ref, tmp / "host.txt", kept_by_level(ref))
    return r, ref


def check_pcal(tmp, name, L=None):
    text, invs, consts, cons, deadlock = contshim.module(name)
    host = helpers.ShimProgram(text, invariants=invs, constants=consts, constraints=cons)
    try:
        ref = contshim.checker_reference(host.translated(), consts, invs, constraints=cons, deadlock=deadlock)
        r = contshim.search("pcal", host.params, deadlock=deadlock, dump=tmp / "host.txt", L=L)
    finally:
        host.close()
    compare(name, r, ref, tmp / "host.txt", kept_by_level(ref))
    return r, ref


@pytest.mark.parametrize("name", list(HAND))
def test_hand_lowerings_against_the_oracles_graph(tmp_path, name):
    r, ref = check_hand(tmp_path, name)
    by = {e["name"]: e for e in ref.entries()}
    if name.startswith("ssi"):
        assert by["(expected-to-be-violated predicate)"]["states"] > 0 and all(e["states"] == 0 for n, e in by.items() if n not in ("(expected-to-be-violated predicate)",))
    if name == "voting":
        assert by["Deadlock"]["states"] > 0 and by["Inv"]["states"] == 0
    if name == "pcal_intro":   # the Assert ends the run, behind levels that broke the invariant
        assert ref.entries()[-1]["kind"] == "assert" and by["MoneyInvariant"]["states"] > 0
        assert ref.entries()[-1]["first_level"] > by["MoneyInvariant"]["first_level"] and r["depth"] == ref.fatal_level + 1


@pytest.mark.parametrize("name", PCAL)
def test_compiled_programs_against_the_checker(tmp_path, name):
    r, ref = check_pcal(tmp_path, name)
    by = {e["name"]: e for e in ref.entries()}
    if name == "many_wrongs":
        # several invariants at once; Both is shadowed: states break it, none as its first invariant
        assert all(by[n]["states"] > 0 for n in ("LockFree", "Small", "Fresh", "Deadlock")) and by["Both"]["states"] == 0
        assert sum(1 for k in ref.kept if not contshim_both_holds(ref.text[k])) > 0
        assert r["distinct"] == len(ref.text)   # nothing fatal: the whole graph
    if name == "init_breaks":
        assert by["Positive"]["first_level"] == 1 and by["Low"]["states"] > 0
    if name == "outside_only":
        assert by["Under"]["states"] == 0 and by["Under"]["outside"] > 0


def contshim_both_holds(text):
    """Both == y < 3 \\/ x < N of many_wrongs (N = 3), read off a state's text"""
    import re
    x, y = int(re.search(r"/\\ x = (\d+)", text).group(1)), int(re.search(r"/\\ y = (\d+)", text).group(1))
    return y < 3 or x < 3


def test_the_modules_in_the_tree_carry_their_translation():
    """specs_continue/*.tla are checked by TLC too: the translation between the markers is the front end's"""
    for name in PCAL:
        text = (contshim.SPECS / f"{name}.tla").read_text()
        assert "\\* BEGIN TRANSLATION" in text and "VARIABLES" in text
        body = text[text.index("\\* BEGIN TRANSLATION"):text.index("\\* END TRANSLATION")]
        assert "Next ==" in body and "Spec ==" in body, name


# ------------------------------------------------------------------------------------------------ mutants
# name: (header, its text, the replacement, the model that must fail, what the failure must say)
MUTANTS = {
    "parentless-skipped": ("violations.h", "if (!has_parent) st = S::init_status(prm, self);", "if (!has_parent) st = 0u;", ("pcal", "init_breaks"), "Positive."),
    "outside-is-state": ("violations.h", "return r.what == VIOL_P_OUTSIDE ? 1 : -1;", "return r.what == VIOL_P_OUTSIDE ? 0 : -1;", ("pcal", "outside_only"), "Under.states"),
    "fatal-not-separated": ("violations.h", "return r.what == VIOL_P_FATAL; }", "return r.flagged; }", ("hand", "pcal_intro"), "MoneyInvariant."),
}


def test_mutants_are_killed(tmp_path):
    helpers.build_shim()

    def build(name):
        return contshim.build_contshim(csrc=testlib.mutant_tree(tmp_path, name, MUTANTS[name][:3]), out=tmp_path / name / "_build")
    for name, so in testlib.build_mutants(MUTANTS, build).items():
        _, _, _, (kind, model), says = MUTANTS[name]
        d = tmp_path / name / "run"
        d.mkdir()
        with pytest.raises(AssertionError) as e:
            (check_hand if kind == "hand" else check_pcal)(d, model, L=contshim.load(so))
            pytest.fail(f"mutant {name} survives", pytrace=False)
        assert says in str(e.value), (name, str(e.value)[:300])
    # ... and the product's own header passes where they fail
    for kind, model in sorted({m[3] for m in MUTANTS.values()}):
        d = tmp_path / f"product_{model}"
        d.mkdir()
        (check_hand if kind == "hand" else check_pcal)(d, model)


# ------------------------------------------------------------------------------------------------ the command line
@pytest.fixture(scope="module")
def mc():
    import tla_rust_amd.build as b
    b.build()
    return b.CLI


@pytest.mark.parametrize("other", [["-gpus", "2"], ["-simulate"], ["-recover", "x.ck"], ["-checkpoint", "x.ck"]])
def test_continue_is_refused_by_name_with(mc, other):
    p = subprocess.run([str(mc), str(contshim.SPECS / "many_wrongs.tla"), "-continue"] + other, capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and f"mc: -continue is not available with {other[0]}" in p.stderr, (p.returncode, p.stderr)


def test_continue_is_in_the_usage_text(mc):
    p = subprocess.run([str(mc), "-help"], capture_output=True, text=True, timeout=60)
    assert "[-continue]" in p.stderr and "past violated invariants and deadlocks" in p.stderr


def test_a_host_evaluated_module_is_refused(mc, tmp_path):
    """a module without a GPU lowering is searched on the host, which ends at its first error: -continue is refused, by name, before any
    device is touched; without the option the same module is checked"""
    (tmp_path / "Tiny.tla").write_text("---- MODULE Tiny ----\nEXTENDS Naturals\nVARIABLE x\nInit == x = 0\nNext == x' = (x + 1) % 3\nSmall == x < 2\n====\n")
    (tmp_path / "Tiny.cfg").write_text("INIT Init\nNEXT Next\nINVARIANT Small\n")
    p = subprocess.run([str(mc), str(tmp_path / "Tiny.tla"), "-continue", "-noprogress"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "-continue is not available for a module evaluated on the host" in p.stderr and p.stdout == "", (p.stdout, p.stderr)
    p = subprocess.run([str(mc), str(tmp_path / "Tiny.tla"), "-noprogress"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 12 and "Error: Invariant Small is violated." in p.stdout, (p.stdout, p.stderr)


def test_the_binding_knows_the_flag_and_the_structs(mc):
    import ctypes
    import inspect
    import tla_rust_amd.binding as b
    assert b.MC_F_CONTINUE == 1 << 26 and "keep_going" in inspect.signature(b.Engine.__init__).parameters
    for sym in ("mc_engine_violations", "mc_engine_violation_trace", "mc_invariant_name"):
        assert hasattr(b.lib(), sym), sym
    assert ctypes.sizeof(b.Violation) == 40 and ctypes.sizeof(b.ViolationsInfo) == 16
    assert "#define MC_F_CONTINUE 67108864u" in (ROOT / "include" / "tlamc.h").read_text()
