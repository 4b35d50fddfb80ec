"""The behaviour rule on the host (tla_rust_amd/csrc/behaviour.h through tests/_behshim, no GPU) against a plain reference over the
oracle's state graph (tests/behaviours.py): every path of the graph is accepted with one candidate under a full mask, a path with one
observation swapped for a non-successor is rejected exactly there, with `pc` hidden the candidate sets equal the reference's set for
set, mc_program_observe gives the mask of the named variables' cells, and the models of specs_behaviours/ give the figures their
headers state; mc_state_parse is the inverse of mc_state_format on every reachable state and gives that mask for partial texts; `mc
-behaviours` refuses the options it does not go with.  Five one-line mutants of behaviour.h are each caught by a named case.

Nothing here needs a GPU; tests/test_gpu_behaviours.py checks that the device kernel gives what this host build gives."""
import sys
from functools import lru_cache
from pathlib import Path

import pytest

import behaviours
import behshim
import helpers
import simgraph
import testlib

ROOT = helpers.ROOT
sys.path.insert(0, str(ROOT / "oracle"))
SB = ROOT / "specs_behaviours"
RAFT_SMALL = [2, 2, 2, 9, 1, 3, 64, 0, 0, 64]   # specs/MCraft_small.cfg as mc_resolve_files lowers it
# name: (spec, the lowering's parameters, the oracle's)
HAND = {
    "pcal_intro": ("pcal_intro", [0, 1, 20, 2], [0, 1, 20, 2]),
    "atomic_add3": ("atomic_add", [3], [3]),
    "raft_small": ("raft", RAFT_SMALL, helpers.raft_oracle_params(RAFT_SMALL)),
    "ssi2x1": ("ssi", [2, 1, 127, 0], [2, 1, 127, 0]),
}
# name: (module, cfg, invariants, constants)
PROGRAMS = {
    "peterson": ("specs/pluscal/peterson.tla", "specs/pluscal/peterson.cfg", ["MutualExclusion", "TurnInRange"], {}),
    "two_phase_soup": ("specs/pluscal/two_phase_soup.tla", "specs/pluscal/two_phase_soup.cfg",
                       ["Consistent", "OneDecision", "PreparedWereSent", "KnownMessages", "SoupIsSmall"], {"RM": 3, "Hasty": False}),
}
MAX_LEN = 6


@lru_cache(maxsize=None)
def program(tla, cfg):
    """a compiled program (the product's host front-end: no GPU), kept for the whole run — nobody changes it"""
    import tla_rust_amd as amd
    return amd.Program((ROOT / tla).read_text(), (ROOT / cfg).read_text())


@lru_cache(maxsize=None)
def graph(name):
    if name in HAND:
        import tempfile
        spec, _, oparams = HAND[name]
        with tempfile.TemporaryDirectory() as d:
            helpers.oracle_graph_files(spec, list(oparams), Path(d) / "states.txt", Path(d) / "edges.txt")
            return simgraph.from_oracle_files(Path(d) / "states.txt", Path(d) / "edges.txt")
    from tla_eval import Checker
    tla, cfg, invs, consts = PROGRAMS[name]
    return simgraph.from_checker(Checker(program(tla, cfg).translated(), constants=consts), invariants=invs)


def model(name, L=None):
    if name in HAND:
        return behshim.Model(HAND[name][0], HAND[name][1], L)
    return behshim.Model("pcal", program(*PROGRAMS[name][:2]).params, L)


class Rows:
    """state text -> row of a model, found along the paths that are asked for (the lowering's own successors, formatted)"""

    def __init__(self, m):
        self.m, self.next, self.init = m, {}, {}
        for r in m.inits():
            self.init.setdefault(m.fmt(r), r)

    def of_path(self, texts):
        row = self.init[texts[0]]
        out = [row]
        for t in texts[1:]:
            if row not in self.next:
                self.next[row] = {}
                for _, _, s in self.m.successors(row):
                    if s is not None:
                        self.next[row].setdefault(self.m.fmt(s), s)
            row = self.next[row][t]
            out.append(row)
        return out


@lru_cache(maxsize=None)
def rows_of(name):
    return Rows(model(name))


@lru_cache(maxsize=None)
def all_paths(name):
    return tuple(p for n in range(1, MAX_LEN + 1) for p in behaviours.paths(graph(name), n))


ALL = list(HAND) + list(PROGRAMS)


@pytest.mark.parametrize("name", ALL)
def test_every_path_is_accepted_with_one_candidate(name):
    g, m, rows = graph(name), model(name), rows_of(name)
    paths = all_paths(name)
    assert len(paths) > MAX_LEN and max(map(len, paths)) == MAX_LEN
    got = m.check([rows.of_path(p) for p in paths])
    print(name, len(paths), "paths")
    bad = [(p, v) for p, v in zip(paths, got) if (v["verdict"], v["step"], v["candidates"], v["peak"]) != ("accepted", len(p), 1, 1)]
    assert not bad, bad[:2]
    # ... and every counter is the reference's (a spread of the paths: the reference is Python)
    for p, v in list(zip(paths, got))[::max(1, len(paths) // 200)]:
        assert v == behaviours.check(g, list(p))[0], p


@pytest.mark.parametrize("name", ALL)
def test_a_swapped_observation_is_rejected_exactly_there(name):
    g, m, rows = graph(name), model(name), rows_of(name)
    paths = [p for p in all_paths(name) if len(p) >= 2]
    paths = paths[::max(1, len(paths) // 150)]
    # a reachable state that is no successor of the state before: taken from the other paths (their rows are known)
    pool = {}
    for p in paths:
        for t, r in zip(p, rows.of_path(p)):
            pool.setdefault(t, r)
    batch, want = [], []
    for k, p in enumerate(paths):
        i = 1 + k % (len(p) - 1)
        succ = {e.text for e in g.succ[p[i - 1]]}
        other = next((t for t in pool if t not in succ), None)
        if other is None:
            continue
        r = rows.of_path(p)
        batch.append(r[:i] + [pool[other]] + r[i + 1:])
        want.append(i)
    assert len(batch) > 10
    got = m.check(batch)
    assert [(v["verdict"], v["step"]) for v in got] == [("rejected", i) for i in want]
    assert all(v["candidates"] == 1 and v["peak"] == 1 for v in got)


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_with_pc_hidden_the_sets_are_the_references(name):
    g, m, rows = graph(name), model(name), rows_of(name)
    prog = program(*PROGRAMS[name][:2])
    names = sorted(set(behaviours.variables_of(g.init[0].text)) - {"pc"})
    mask = prog.observe(names)
    paths = all_paths(name)
    paths = paths[::max(1, len(paths) // 120)]
    wider = 0
    for stutter in (False, True):
        for p in paths:
            want, want_sets = behaviours.check(g, [behaviours.observe(t, names) for t in p], names, stutter)
            got, got_sets, wit = m.sets(rows.of_path(p), mask, stutter)
            assert got == want, (p, stutter)
            assert [{m.fmt(r) for r in s} for s in got_sets] == want_sets, (p, stutter)
            wider += want["peak"] > 1
            # the witness is a path of the graph through the sets, observation by observation
            assert len(wit) == len(got_sets) == want["step"]
            texts = [m.fmt(r) for _, r in wit]
            assert all(t in s for t, s in zip(texts, want_sets)) and wit[0][0] == -1
            for a, b, (slot, _) in zip(texts, texts[1:], wit[1:]):
                assert (slot == -2 and a == b) or (slot >= 0 and b in {e.text for e in g.succ[a]}), (a, b, slot)
    assert wider > 0   # (hiding pc does make some behaviour ambiguous between states)


def test_observe_gives_the_cells_of_the_named_variables():
    import tla_rust_amd as amd
    prog = program(*PROGRAMS["peterson"][:2])
    m = model("peterson")
    names = sorted(behaviours.variables_of(graph("peterson").init[0].text))
    one = {n: prog.observe([n]) for n in names}
    assert all(len(v) == m.W and set(v) <= {0, 255} and any(v) for v in one.values())
    # the variables' cells are disjoint and together they are what observing all of them gives
    total = bytes(m.W)
    for v in one.values():
        assert not any(a & b for a, b in zip(total, v))
        total = bytes(a | b for a, b in zip(total, v))
    assert total == prog.observe(names)
    # a row differs from a successor exactly inside the cells of the variables whose text changed
    r0 = m.inits()[0]
    for _, _, r1 in m.successors(r0):
        a, b = behaviours.variables_of(m.fmt(r0)), behaviours.variables_of(m.fmt(r1))
        changed = bytes(m.W)
        for n in names:
            if a[n] != b[n]:
                changed = bytes(x | y for x, y in zip(changed, one[n]))
        assert all(x == y or c for x, y, c in zip(r0, r1, changed))
        assert all(any(x != y for x, y, c in zip(r0, r1, one[n]) if c) for n in names if a[n] != b[n])
    with pytest.raises(amd.McError, match="no variable `nosuch`"):
        prog.observe(["turn", "nosuch"])


# ------------------------------------------------------------------------------------------------ the models of specs_behaviours/
def sb_program(stem, cfg=None):
    return program(f"specs_behaviours/{stem}.tla", f"specs_behaviours/{cfg or stem}.cfg")


def first_walk(m, n):
    """n states from the first initial state, always through the lowest enabled slot that changes the row"""
    rows = [m.inits()[0]]
    while len(rows) < n:
        rows.append(next(t for _, _, t in m.successors(rows[-1]) if t is not None and t != rows[-1]))
    return rows


def v(verdict, step, candidates, peak, generated, outside=0, errors=0):
    return dict(verdict=verdict, step=step, candidates=candidates, peak=peak, generated=generated, outside=outside, errors=errors)


@lru_cache(maxsize=None)
def case_inputs():
    """{case: (program parameters, batch, mask, stutter)}: the cases the models of specs_behaviours/ are for, and the mutants are caught by"""
    out = {}
    p = sb_program("hidden_choice")
    m = behshim.Model("pcal", p.params)
    w, x = first_walk(m, 4), p.observe(["x"])
    out["hidden_choice 64: a full set is no ambiguity"] = (p.params, [w[:1], w[:2], w], x, False)
    p65 = sb_program("hidden_choice", "hidden_choice_65")
    out["hidden_choice 65: ambiguous at 0"] = (p65.params, [w[:2]], p65.observe(["x"]), False)
    p = sb_program("hidden_late")
    w = first_walk(behshim.Model("pcal", p.params), 4)
    out["hidden_late 64"] = (p.params, [w[:2], w[:3], w], p.observe(["x"]), False)
    p65 = sb_program("hidden_late", "hidden_late_65")
    out["hidden_late 65: ambiguous at 1"] = (p65.params, [w[:1], w[:3]], p65.observe(["x"]), False)
    p = sb_program("diamond")
    w, x = first_walk(behshim.Model("pcal", p.params), 2), p.observe(["x"])
    out["diamond: x alone is observed"] = (p.params, [w], x, False)
    out["diamond: a repeated observation without the stutter flag"] = (p.params, [[w[0], w[0], w[1]]], x, False)
    out["diamond: a repeated observation with it"] = (p.params, [[w[0], w[0], w[1], w[1]]], x, True)
    p = sb_program("beyond")
    out["beyond: steps that leave the CONSTRAINT"] = (p.params, [first_walk(behshim.Model("pcal", p.params), 5)], None, False)
    p = sb_program("failing_step")
    w, xm = first_walk(behshim.Model("pcal", p.params), 2), p.observe(["x"])
    third = bytearray(w[1])   # the log's third entry says x = 2: what the assignments alone would give
    third[xm.index(255):xm.index(255) + 4] = (2).to_bytes(4, "little")
    out["failing_step: the only matching step fails its Assert"] = (p.params, [w + [bytes(third)]], xm, False)
    p = program("specs_cfgmore/ghost_history.tla", "specs_cfgmore/ghost_history.cfg")
    m = behshim.Model("pcal", p.params)
    r = [m.inits()[0]]
    for worker in (0, -1, 0, -1):   # rd, rd, wr, wr: the lowest enabled slot is worker 1's, the highest worker 2's
        r.append([t for _, _, t in m.successors(r[-1]) if t is not None and t != r[-1]][worker])
    out["ghost_history: two rows with one fingerprint"] = (p.params, [r], p.observe(["x", "t"]), False)
    return out


def named_cases(L=None):
    """{case: verdicts} on the library L (None: the product's)"""
    return {name: behshim.Model("pcal", params, L).check(batch, mask, stutter) for name, (params, batch, mask, stutter) in case_inputs().items()}


# what the models' headers state, case by case
EXPECTED = {
    "hidden_choice 64: a full set is no ambiguity": [v("accepted", 1, 64, 64, 64), v("accepted", 2, 32, 64, 128), v("accepted", 4, 8, 64, 176)],
    "hidden_choice 65: ambiguous at 0": [v("ambiguous", 0, 0, 0, 65)],
    "hidden_late 64": [v("accepted", 2, 64, 64, 1 + 64), v("accepted", 3, 64, 64, 1 + 64 + 64 * 64), v("accepted", 4, 64, 64, 1 + 64 + 2 * 64 * 64)],
    "hidden_late 65: ambiguous at 1": [v("accepted", 1, 1, 1, 1), v("ambiguous", 1, 1, 1, 1 + 65)],
    "diamond: x alone is observed": [v("accepted", 2, 1, 2, 2 + 2)],
    "diamond: a repeated observation without the stutter flag": [v("rejected", 1, 2, 2, 2 + 2)],
    "diamond: a repeated observation with it": [v("accepted", 4, 1, 2, 2 + 2 + 2 + 1)],
    "beyond: steps that leave the CONSTRAINT": [v("accepted", 5, 1, 1, 5, outside=2)],
}


def test_the_models_of_specs_behaviours():
    c = named_cases()
    for name, want in EXPECTED.items():
        assert c[name] == want, name
    got = c["failing_step: the only matching step fails its Assert"][0]
    assert (got["verdict"], got["step"], got["errors"], got["candidates"]) == ("rejected", 2, 1, 1)
    got = c["ghost_history: two rows with one fingerprint"][0]
    assert (got["verdict"], got["step"], got["candidates"]) == ("accepted", 5, 4), got


# ------------------------------------------------------------------------------------------------ text
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_parse_is_the_inverse_of_format(name):
    """mc_state_parse(mc_state_format(s)) == s with a full mask on every reachable state; a text without its pc conjunct gives the row
    with pc's cells zero and mc_program_observe's mask of the other variables"""
    import tla_rust_amd as amd
    prog, m = program(*PROGRAMS[name][:2]), model(name)
    by_text, _ = m.reachable()
    assert len(by_text) > 20
    names = sorted(behaviours.variables_of(next(iter(by_text))))
    full, nopc = prog.observe(names), prog.observe([n for n in names if n != "pc"])
    for row in by_text.values():
        text = amd.state_format("pcal", prog.params, row)
        assert amd.binding.state_parse("pcal", prog.params, text) == (row, full), text
        part = "\n".join(ln for ln in text.split("\n") if not ln.startswith("/\\ pc "))
        assert part != text
        assert amd.binding.state_parse("pcal", prog.params, part) == (bytes(a & b for a, b in zip(row, nopc)), nopc), part


def test_parse_refuses_what_is_no_state():
    import tla_rust_amd as amd
    prog = program(*PROGRAMS["peterson"][:2])
    for text, why in (("/\\ nosuch = 1", "no variable `nosuch`"), ("/\\ turn = TRUE", "turn: .*a number is expected"),
                      ("/\\ pc = (0 :> \"nolabel\" @@ 1 :> \"nolabel\")", "knows no string"), ("turn = 1", "is expected"),
                      ("/\\ turn = ", "turn: ")):
        with pytest.raises(amd.McError, match=why) as e:
            amd.binding.state_parse("pcal", prog.params, text)
        assert e.value.code == -8, text
    with pytest.raises(amd.McError) as e:
        amd.binding.state_parse("atomic_add", [3], "/\\ x = 1")
    assert e.value.code == -9


RECORDS = """---- MODULE records ----
EXTENDS Naturals
(* --algorithm records
variables flag_x = 0, r = [a |-> 1, b |-> 2];
process P = 0
begin
  s: r.a := r.b;
     flag_x := 1;
end process
end algorithm *)
====
"""


def test_observe_a_record_stands_for_its_fields_and_a_prefix_for_nothing():
    import tla_rust_amd as amd
    prog = amd.Program(RECORDS, "SPECIFICATION Spec\n")
    try:
        assert prog.observe(["r"]) == bytes(a | b for a, b in zip(prog.observe(["r_a"]), prog.observe(["r_b"]))) and any(prog.observe(["r"]))
        assert not any(a & b for a, b in zip(prog.observe(["r"]), prog.observe(["flag_x"])))
        with pytest.raises(amd.McError, match="no variable `flag`"):   # (flag_x is no field of a record `flag`)
            prog.observe(["flag"])
    finally:
        prog.close()


@pytest.mark.parametrize("other", [["-simulate"], ["-gpus", "2"], ["-recover", "x.ck"], ["-checkpoint", "x.ck"], ["-dump", "x.txt"], ["-coverage"], ["-continue"]])
def test_cli_behaviours_refusals(other):
    import subprocess
    mc = ROOT / "tla_rust_amd" / "_build" / "mc"
    p = subprocess.run([str(mc), str(SB / "diamond.tla"), "-behaviours", "log.txt", *other], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and f"{other[0]} is not available with -behaviours" in p.stderr, (p.stdout, p.stderr)


# ------------------------------------------------------------------------------------------------ mutants
# name: (text of behaviour.h, its replacement, the named case that must catch it)
MUTANTS = {
    "mask-ignored": ("(mask ? mask[w] : ~0ull)", "~0ull", "diamond: x alone is observed"),
    "no-row-compare": ("if (m.fp == fp && beh_same_row(CWordRef{m.row.data(), 1}, CWordRef{row, 1}, W)) {", "if (m.fp == fp) {",
                       "ghost_history: two rows with one fingerprint"),
    "outside-dropped": ("return st & ST_OUT_OF_MODEL ? BEH_STEP_OUTSIDE : BEH_STEP;", "return st & ST_OUT_OF_MODEL ? BEH_NO_STEP : BEH_STEP;",
                        "beyond: steps that leave the CONSTRAINT"),
    "stutter-unasked": ("if ((flags & MC_BEH_F_STUTTER) && beh_match(s, obs, mask, W))", "if (beh_match(s, obs, mask, W))",
                        "diamond: a repeated observation without the stutter flag"),
    "ambiguous-at-64": ("if (nxt.size() + 1 > MC_BEH_MAX_CANDIDATES) {", "if (nxt.size() + 1 >= MC_BEH_MAX_CANDIDATES) {",
                        "hidden_choice 64: a full set is no ambiguity"),
}


def test_mutants_are_caught(tmp_path):
    helpers.build_shim()

    def build(name):
        return behshim.build(csrc=testlib.mutant_tree(tmp_path, name, ("behaviour.h", *MUTANTS[name][:2])), out=tmp_path / name / "_build")
    good = named_cases()
    for name, so in testlib.build_mutants(MUTANTS, build).items():
        bad = named_cases(behshim.load(so))
        assert bad[MUTANTS[name][2]] != good[MUTANTS[name][2]], f"mutant {name} survives its case"
