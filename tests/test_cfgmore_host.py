"""cfg VIEW and ACTION_CONSTRAINT for compiled PlusCal programs, without a GPU: the front end accepts the cfgs of
specs_cfgmore/ and refuses what it must; the compiled program — on the host build of the interpreter and as generated code — agrees with
the reference of tests/cfgmore.py and with the product's own host evaluator; a cfg without the statements compiles to what it did; and
four one-line mutants of the new code are each caught by the model written for it."""
import ctypes as C
import json
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

import cfgmore
import helpers
import testlib

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

COUNTS = ("distinct", "generated", "depth", "verdict", "trace_len", "levels")


@pytest.fixture(scope="module")
def amd():
    import tla_rust_amd as amd
    amd.lib()
    return amd


def shim_run(lib, params, dump):
    d = helpers.spec_desc("pcal", params)
    res = helpers.ShimResult()
    lib.shim_run.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_uint64, C.c_uint64, C.c_int, C.c_char_p, C.POINTER(helpers.ShimResult)]
    assert lib.shim_run(C.byref(d), 0, 0, 1, str(dump).encode(), C.byref(res)) == 0
    return dict(distinct=res.distinct, generated=res.generated, depth=res.depth, verdict=helpers.VERDICTS[res.verdict], trace_len=res.trace_len,
                levels=[res.level_distinct[i] for i in range(res.levels)], fp_mismatch=res.fp_mismatch)


def check_model(name, tmp_path, lib=None):
    """the host build of the interpreter (`lib`: a mutant's) against the reference: counts, verdict, and the view values per level"""
    prog, ref, want = cfgmore.load(name)
    dump = tmp_path / f"{name}.dump"
    got = shim_run(lib or helpers.shim_lib(), prog.params, dump)
    print(name, {k: got[k] for k in COUNTS}, {k: want[k] for k in COUNTS})
    assert got["fp_mismatch"] == 0, ("a stored row does not carry the fingerprint it was looked up by", name)
    assert {k: got[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, ("counts differ from the reference", name)
    assert cfgmore.level_views_of_dump(ref, dump) == want["level_views"], ("view values per level differ from the reference", name)


def test_programs_expose_their_view_and_action_constraints(amd):
    expect = {"ghost_history": ("<<x, pc, t>>", []), "parity_view": ("<<(x % 2), pc>>", []), "ac_two": (None, ["Slow", "YUp"]),
              "ac_monotone": (None, ["Up"]), "wide": ("<<x, pc, c>>", ["Gentle"]), "ac_deadlock_twin": (None, []),
              "view_kinds": ("<<r_cnt, r_flag, q, msgs, pc>>", []), "ac_soup": (None, ["Keep"])}   # (a record in a view: its fields' variables)
    for name in cfgmore.MODELS:
        prog = cfgmore.load(name)[0]
        if name in expect:
            assert (prog.view, prog.action_constraints) == expect[name], name
        cfg = cfgmore.read_cfg(cfgmore.texts(name)[1])
        assert (prog.view is not None) == bool(cfg["VIEW"]) and prog.action_constraints == cfg["ACTION_CONSTRAINT"], name
    L = amd.binding.lib()
    assert L.mc_program_view(None) is None and L.mc_program_action_constraint(None, 0) is None
    assert L.mc_program_action_constraint(cfgmore.load("ac_two")[0]._h, 2) is None


def test_both_spellings_of_the_statement(amd):
    tla, cfg = cfgmore.texts("ac_monotone")
    for kw in ("ACTION_CONSTRAINTS", "ACTION-CONSTRAINT", "ACTION-CONSTRAINTS"):
        p = amd.Program(tla, cfg.replace("ACTION_CONSTRAINT", kw))
        assert p.action_constraints == ["Up"]
        p.close()


@pytest.mark.parametrize("name", list(cfgmore.REFUSED))
def test_refusals_name_their_reason(amd, name):
    with pytest.raises(amd.McError) as e:
        amd.Program(*cfgmore.texts(name))
    assert cfgmore.REFUSED[name] in str(e.value), str(e.value)


def test_termination_under_a_view_is_refused_with_the_word(amd):
    p = amd.Program(*cfgmore.texts("termination_view"))
    assert p.view == "<<x, pc>>" and p.live_refusal and "VIEW" in p.live_refusal
    q = amd.Program(cfgmore.texts("termination_view")[0], "SPECIFICATION Spec\nPROPERTY Termination\n")
    assert q.live_refusal is None and q.view is None


def test_a_single_record_variable_as_the_view(amd):
    tla, _ = cfgmore.texts("view_kinds")
    p = amd.Program(tla.replace("View == <<r, q, msgs, pc>>", "View == r"), "SPECIFICATION Spec\nVIEW View\n")
    assert p.view == "<<r_cnt, r_flag>>"
    p.close()


def test_an_evaluation_error_inside_an_action_constraint_is_a_spec_error(tmp_path):
    """ac_error: x' \\div x on the first step, x = 0 — reported at the state being expanded (trace length 1), as an error inside an invariant is"""
    prog = cfgmore.compiled("ac_error")
    got = shim_run(helpers.shim_lib(), prog.params, tmp_path / "d")
    assert (got["verdict"], got["trace_len"], got["distinct"], got["generated"]) == ("spec-error", 1, 1, 2), got
    (tmp_path / "ac_error.tla").write_text(prog.translated())
    r = helpers.tlaeval_run(tmp_path / "ac_error.tla", cfgmore.DIR / "ac_error.cfg")   # the host evaluator's opinion: an error too
    assert r["rc"] != 0 or helpers.VERDICTS[r["verdict"]] == "spec-error", r


def test_a_prime_outside_an_action_constraint_is_refused(amd):
    tla, _ = cfgmore.texts("ac_monotone")
    with pytest.raises(amd.McError) as e:
        amd.Program(tla, "SPECIFICATION Spec\nINVARIANT Up\n")
    assert "outside an ACTION_CONSTRAINT" in str(e.value)


@pytest.mark.parametrize("name", list(cfgmore.MODELS))
def test_the_reference_shows_what_the_model_was_written_for(name):
    m, (prog, ref, r) = cfgmore.MODELS[name], cfgmore.load(name)
    assert (r["distinct"], r["depth"], r["verdict"]) == (m.distinct, m.depth, m.verdict)
    assert sum(r["levels"]) == r["distinct"] or r["verdict"] != "ok"
    assert all(len(v) == n for v, n in zip(r["level_views"], r["levels"]))   # one stored state per view value
    if ref.acons:
        assert r["refused"] > 0, "no transition of the model is refused: the action constraint shows nothing"


def test_what_each_model_shows():
    load = cfgmore.load
    # the ghosts are really left out: without the view ghost_history has more states, and the viewed search visits exactly the views of the unviewed one
    prog, ref, r = load("ghost_history")
    plain = cfgmore.Reference(prog, cfgmore.texts("ghost_history")[1], with_view=False).run()
    assert plain["distinct"] > r["distinct"] and plain["depth"] == r["depth"]
    both = cfgmore.Reference(prog, cfgmore.texts("ghost_history")[1])
    earlier = set()
    for k, lines in enumerate(plain["level_lines"]):   # a congruence: level k of the viewed search = the views that level k of the unviewed one reaches first
        views = {both.view_of_text(s) for s in lines}
        assert views - earlier == r["level_views"][k]
        earlier |= views
    # ghost_unbounded: the quotient of ghost_history (n plays no part); its unviewed graph is cut by CONSTRAINT Small (K >= the depth)
    prog_u, _, ru = load("ghost_unbounded")
    assert ru["levels"] == r["levels"] and cfgmore.read_cfg(cfgmore.texts("ghost_unbounded")[1])["CONSTANT"]["K"] >= ru["depth"]
    cut = cfgmore.Reference(prog_u, cfgmore.texts("ghost_unbounded")[1], with_view=False, extra_constraints=["Small"]).run()
    assert cut["distinct"] > ru["distinct"] and cut["depth"] > ru["depth"]   # (the counter goes on where the views repeat)
    uref = cfgmore.Reference(prog_u, cfgmore.texts("ghost_unbounded")[1])
    assert {uref.view_of_text(s) for lines in cut["level_lines"] for s in lines} == set().union(*ru["level_views"])
    # view_init: two initial states are generated, one is stored
    _, ref_i, ri = load("view_init")
    assert ri["levels"][0] == 1 and len(list(ref_i.ck.initial_states())) == 2
    # ac_monotone: the constraint changes the reachable set and the per-level counts
    prog_m, _, rm = load("ac_monotone")
    free = cfgmore.Reference(prog_m, cfgmore.texts("ac_monotone")[1], with_acons=False).run()
    assert free["levels"][:3] != rm["levels"] and free["distinct"] > rm["distinct"] and free["generated"] > rm["generated"]
    # ac_two: the violation comes from a REFUSED transition out of the initial state (trace length 2); without Slow's refusal it would be stored
    _, _, r2 = load("ac_two")
    assert (r2["verdict"], r2["violated"], r2["trace_len"]) == ("invariant", "Inv", 2)
    assert not any("x = 3" in s for s in r2["level_lines"][1])
    # ac_deadlock and its CONSTRAINT twin agree
    a, b = load("ac_deadlock")[2], load("ac_deadlock_twin")[2]
    assert {k: a[k] for k in COUNTS} == {k: b[k] for k in COUNTS}
    # wide: 17 slots per state, two levels wider than 256 states
    prog_w, _, rw = load("wide")
    assert prog_w.ninst == 4 and sum(1 for n in rw["levels"] if n > 256) >= 2


@pytest.mark.parametrize("name", [n for n, m in cfgmore.MODELS.items() if m.congruent])
def test_stored_states_of_a_congruent_view_are_states_of_the_unviewed_graph(name, tmp_path):
    """... on the same level (the view is a congruence: a representative is reached as early as its view)"""
    prog, ref, _ = cfgmore.load(name)
    extra = ["Small"] if name == "ghost_unbounded" else []
    plain = cfgmore.Reference(prog, cfgmore.texts(name)[1], with_view=False, extra_constraints=extra).run()
    dump = tmp_path / "d"
    shim_run(helpers.shim_lib(), prog.params, dump)
    for ln in dump.read_text().splitlines():
        lv, _, text = ln.partition(" ")
        assert text in plain["level_lines"][int(lv[1:]) - 1], (name, ln)


@pytest.mark.parametrize("name", list(cfgmore.MODELS))
def test_the_interpreter_on_the_host_equals_the_reference(name, tmp_path):
    check_model(name, tmp_path)


def test_no_host_walk_of_the_simulation_takes_a_refused_step(tmp_path):
    """tests/simgraph.py judges the host build's random walks against the reference's graph, in which a refused transition is an edge
    that cannot be walked: every walk of ac_monotone is legal and ends where all successors are refused"""
    import simgraph
    from test_simulate_graph import check
    prog, ref, _ = cfgmore.load("ac_monotone")
    ends, _, _ = check(tmp_path, cfgmore.sim_graph(ref), "pcal", prog.params, 5, 200, 12, True)
    assert ends[simgraph.END_OUT_OF_MODEL] == 200


class _Handle:   # what helpers.program_codegen needs of a program
    def __init__(self, prog):
        self.h = prog.params[0]


@pytest.mark.parametrize("name,pack", [("ghost_history", "1"), ("ac_records", "1"), ("ac_two", "1"), ("wide", "1"), ("wide", "0")])
def test_generated_code_equals_the_interpreter(name, pack, monkeypatch):
    """tests/_gen/harness.cpp's route, with the interpreter that knows the statements in SpecVm's place (tests/_cfgmore/harness_cfg.cpp):
    generated code against it on every reachable state and slot — statuses (the refusals among them), rows, fingerprints (the view's
    among them) — and the search's counts against the reference"""
    monkeypatch.setenv("TLAMC_JIT_PACK", pack)
    prog, _, want = cfgmore.load(name)
    text = helpers.program_codegen(_Handle(prog))
    assert ("NACON" in text) == ("run_acon" in text) == bool(prog.action_constraints)
    assert ("VIEW_WORDS" in text) == ("view_words" in text) == (prog.view is not None)
    assert ("PACKED = true" in text) == (pack == "1" and name != "ac_two")   # (ac_two's cells have no bounded range: packing saves no word)
    g = cfgmore.gen_check(prog)
    print(name, pack, g)
    assert g["mismatches"] == 0, g
    if want["verdict"] == "ok":   # (the harness searches on past a violation: ac_two is compared state by state and slot by slot only)
        assert (g["distinct"], g["generated"], g["depth"]) == (want["distinct"], want["generated"], want["depth"])


def test_the_host_evaluator_gives_the_same_counts(tmp_path):
    """the product's own host evaluator (tlaeval.cpp: key_of, in_actions) on the translated module and the same cfg: a second, differently
    built opinion"""
    for name in cfgmore.MODELS:
        prog, _, want = cfgmore.load(name)
        (tmp_path / f"{name}.tla").write_text(prog.translated())
        r = helpers.tlaeval_run(tmp_path / f"{name}.tla", cfgmore.DIR / f"{name}.cfg")
        assert r["rc"] == 0, (name, r)
        assert (r["distinct"], r["generated"], r["depth"], r["levels"]) == (want["distinct"], want["generated"], want["depth"], want["levels"]), name
        assert helpers.VERDICTS[r["verdict"]] == want["verdict"], name


def test_a_cfg_without_the_statements_compiles_to_what_it_did(amd):
    """image, the scalar fields of VmParams and generated header of every cfg under specs/pluscal and specs_liveness are those recorded
    from the front end before it knew the statements (tests/golden/liveprops_images.json: the checkpoint identity hashes the image and
    those fields); and a program WITH them keeps the image of the program without them as a prefix, header words included"""
    import test_liveprops_host as t
    golden = json.loads(t.GOLDEN.read_text())
    checked = 0
    for tla, cfg in t.old_cfgs():
        try:
            p = amd.Program(tla.read_text(), cfg.read_text())
        except amd.McError:
            assert golden[str(cfg.relative_to(ROOT))] is None, cfg
            continue
        assert p.view is None and p.action_constraints == []
        image, fields = t.image_of(p)
        assert t.digest(image, fields, t.header_of(amd, p)) == golden[str(cfg.relative_to(ROOT))], cfg
        checked += 1
        p.close()
    assert checked >= 30
    tla, cfg = cfgmore.texts("wide")
    with_, without = amd.Program(tla, cfg), amd.Program(tla, "SPECIFICATION Spec\n")
    (a, fa), (b, fb) = t.image_of(with_), t.image_of(without)
    assert len(a) > len(b)
    n_hdr = 24   # (VMH_SIZE: magic .. NCON)
    from array import array
    wa, wb = list(array("i", a)), list(array("i", b))
    code_len = next(i for i in range(n_hdr) if wa[i] != wb[i])   # the only header word that differs: the length
    assert (wa[code_len], wb[code_len]) == (len(wa), len(wb)) and wa[:code_len] + wa[code_len + 1:len(wb)] == wb[:code_len] + wb[code_len + 1:]
    h_with, h_without = t.header_of(amd, with_), t.header_of(amd, without)
    assert "run_acon" in h_with and "view_words" in h_with and "run_acon" not in h_without and "VIEW" not in h_without


# name: (its text in spec_vm_cfg.h, the replacement, the model that must catch it)
MUTANTS = {
    "old-and-new-swapped": ("const_cast<int32_t *>(cur), res, aux, v);",
                            "const_cast<int32_t *>(v), res, aux, cur);", "ac_monotone"),
    "refused-successor-stored": ("if (!res) return ST_OUT_OF_MODEL;", "if (!res) return 0;", "ac_indexed"),
    "last-component-not-hashed": ("for (int k = 0; k < x[VMX_NVIEW]; ++k) {", "for (int k = 0; k + 1 < x[VMX_NVIEW]; ++k) {", "ghost_history"),
    "view-not-applied-to-initial-states": ("if (vm_ext(p)[VMX_NVIEW]) { uint64_t fp; (void)fp_view(p, v, fp); return fp; }", "", "view_init"),
}


def test_mutants_of_the_new_code_are_caught(tmp_path):
    def build(name):
        top = tmp_path / name
        d = testlib.mutant_tree(tmp_path, name, ("spec_vm_cfg.h", *MUTANTS[name][:2]), also=testlib.FRONT_END)
        (top / "tests" / "_shim").mkdir(parents=True)   # (shim.cpp includes ../../tla_rust_amd/csrc/...: the copy reads the mutant's)
        shutil.copy(ROOT / "tests" / "_shim" / "shim.cpp", top / "tests" / "_shim" / "shim.cpp")
        so = top / "libshim_mutant.so"
        # (-Bsymbolic: the mutant's own copies of the interpreter's functions, whatever library of the same names the process has loaded)
        subprocess.run(["g++", "-O0", "-std=c++17", "-fPIC", "-shared", "-w", "-Wl,-Bsymbolic", "-o", str(so), str(top / "tests" / "_shim" / "shim.cpp"),
                        str(d / "pcal.cpp"), str(d / "pcal_compile.cpp"), str(d / "pcal_codegen.cpp")], check=True)
        return so
    for name, so in testlib.build_mutants(MUTANTS, build).items():
        run = tmp_path / name / "run"
        run.mkdir()
        with pytest.raises(AssertionError) as e:
            check_model(MUTANTS[name][2], run, lib=C.CDLL(str(so)))
            pytest.fail(f"mutant {name} survives", pytrace=False)
        assert "differ from the reference" in str(e.value) or "fingerprint it was looked up by" in str(e.value), (name, str(e.value)[:300])
