"""tests/sidemodel.py against the product's own host loops over the table lowering (tests/_sideshim/sidehost.cpp: graph_state, cov_state,
viol_stored_bin / viol_pair / viol_deadlocked, live_edge_unit — the MC_HD rules the kernels run too), on every case
tests/test_gpu_sidepasses.py drives the kernels with; four one-line mutants of the MODEL that this comparison must catch; and the
conditions the cases rely on, so that a GPU test cannot pass because its input was degenerate.  No GPU: the device shim and the five
device mutants are only compiled here (hipcc cross-compiles gfx950)."""
import numpy as np
import pytest

import seenmodel as SM
import sidemodel as M
import sideshim as X
import testlib
from test_gpu_sidepasses import MUTANTS, check_coverage, check_graph, check_violations, graph_want, mutant_libraries
from testlib import survives

CASES = M.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_the_model_is_the_host_loops(name):
    check_graph(name, host=True)
    check_coverage(name, host=True)
    check_violations(name, host=True)


MODEL_MUTANTS = {   # the rule that is wrong -> a case that shows it, and the driver
    "flagged-pairs-are-looked-up": ("graph/statuses", check_graph),
    "any-record-counts": ("coverage/ids-nbins7", check_coverage),
    "outside-is-stored": ("violations/init", check_violations),
    "deadlock-is-no-slots": ("violations/deadlocks", check_violations),
}


@pytest.mark.parametrize("mutant", list(MODEL_MUTANTS))
def test_a_wrong_model_is_caught(mutant, monkeypatch):
    name, check = MODEL_MUTANTS[mutant]
    check(name, host=True)
    monkeypatch.setattr(M, "MUTANT", mutant)
    graph_want.cache_clear()
    try:
        assert not survives(lambda: check(name, host=True))
    finally:
        graph_want.cache_clear()


def test_the_device_shim_and_its_mutants_compile():
    assert X.build().exists()
    for edit in MUTANTS.values():
        testlib.mutant_texts(edit)   # (asserts that its text occurs once and that the replacement differs)
    assert len(MUTANTS) >= 5 and all(so.exists() for so in mutant_libraries().values())


# --------------------------------------------------------------------------------------------------- what the cases are there to hold
def test_the_sizes_chunks_and_ranges_are_what_the_issue_lists():
    graphs = {k: c for k, c in CASES.items() if k.startswith("graph/")}
    assert {c.n for c in graphs.values()} >= {1, 63, 64, 65, 257, 600}
    assert {c.chunk for c in CASES.values()} == {64, 128, 256}
    assert {c.lo for c in CASES.values()} >= {0, 1, 63, 70, 130} and any(c.hi % 64 for c in CASES.values())
    assert all(c.hi % 64 for k, c in CASES.items() if "level-lo" in k)
    assert {c.prm.nbins for c in CASES.values()} >= {2, 7, X.COV_MAX_BINS}
    assert {(c.nbuckets, c.sparse) for c in graphs.values()} >= {(64, False), (64, True), (37, False), (37, True)}
    assert max(s.nslots for c in CASES.values() for s in c.states) >= 40 and all(c.n <= 4000 for c in CASES.values())
    for c in CASES.values():   # several launches per level somewhere, and more than one workgroup
        assert len({s.key for s in c.states}) == c.n
    assert any(c.hi - c.lo > 2 * c.chunk for c in CASES.values()) and any(c.chunk == 256 and c.n > 512 for c in CASES.values())


def test_the_wavefronts_are_as_mixed_as_their_names_say():
    ladder = CASES["graph/ladder"]
    for w in (0, 1):
        assert sorted(s.nslots for s in ladder.states[64 * w:64 * w + 64]) == list(range(64))
    spike = CASES["graph/spike"]
    assert sorted(s.nslots for s in spike.states)[-2:] == [0, 40]
    mixed, uniform = CASES["coverage/mixed"], CASES["coverage/uniform"]
    def per_slot(c):   # distinct actions among a wavefront's lanes, per slot iteration
        return [len({s.slots[j][1] for s in c.states[64:128]}) for j in range(6)]
    assert set(per_slot(uniform)) == {1}
    assert per_slot(mixed)[0::2] == [1, 1, 1] and min(per_slot(mixed)[1::2]) > 1   # they agree in the even iterations only
    for lane in (0, 63):
        c = CASES[f"coverage/one-lane-{lane}"]
        assert {i % 64 for i, s in enumerate(c.states) if any(st & M.EN for st, _, _ in s.slots[:s.nslots])} == {lane}
        assert {i % 64 for i in range(c.hi, c.new_hi) if c.parent[i] < i} == {lane} and c.hi % 64 == 0
    for k, c in CASES.items():   # a walk that forgot idx >= lo would find something to count below lo
        if c.lo % 64:
            assert any(st & M.EN and 0 <= a + 1 < c.prm.nbins for s in c.states[c.lo & ~63:c.lo] for st, a, _ in s.slots[:s.nslots]), k


def test_the_chains_wrap_the_end_of_the_table():
    for nb in (64, 37):
        for sparse in (False, True):
            c = CASES[f"graph/chain-{nb}-{'sparse' if sparse else 'dense'}"]
            words = [int(w) for w in c.table]
            targets = {key for s in c.states for st, _, key in s.slots[:s.nslots] if key}
            wrapped = [k for k in targets if M.find(words, nb, c.slots, k) // c.slots < SM.home(k, nb)]
            assert len(wrapped) >= 3 and any(SM.home(k, nb) == nb - 2 for k in wrapped) and any(k & 0xffffffff == 0xffffffff for k in wrapped)
            assert all((c.table.reshape(nb, c.slots)[b] != 0).all() for b in (nb - 2, nb - 1, 0))   # the buckets the lookups cross are full
            assert sum(1 for s in c.states for st, _, key in s.slots[:s.nslots] if key == 0 and st == M.EN) == 1
            assert graph_want(f"graph/chain-{nb}-{'sparse' if sparse else 'dense'}")["gc_degree"][1] == 1   # ... which is the one thing missing


def test_every_status_word_is_there_stored_and_not():
    c = CASES["graph/statuses"]
    words = [int(w) for w in c.table]
    seen = {(st & 0x7f, M.find(words, c.nbuckets, c.slots, key) != M.ABSENT) for s in c.states[:64] for st, _, key in s.slots[:s.nslots]}
    assert seen == {(st, there) for st in range(128) for there in (False, True)}
    records = {c.states[c.parent[i]].slots[c.pslot[i]][0] & 0x7f for i in range(64, c.n)}
    assert records == set(range(128))


def test_the_inconsistent_cases_break_one_thing_each():
    for what, counter in (("self", 0), ("absent", 1), ("no-index", 1)):
        both, alone = graph_want(f"graph/inconsistent-{what}-both"), graph_want(f"graph/inconsistent-{what}-last-wavefront")
        assert both["gc_fill"][2] >> 16 == 5 and alone["gc_fill"][2] >> 16 == 129
        assert both["gc_degree"][1 - counter] == 0 or what == "self"   # (a lost state's key is also somebody's lost successor)
        if what == "self":
            assert both["gc_degree"][0] == 2 and alone["gc_degree"][0] == 1 and both["gc_degree"][2] & 0xffff == 0xffff
        elif what == "absent":
            assert both["gc_degree"][:2].tolist() == [0, 2] and both["gc_fill"][1] == 4 and both["gc_degree"][2] == (5 << 16 | 1)
        else:
            assert both["gc_degree"][:3].tolist() == [0, 0, M.ALL] and both["gc_fill"][1] == 2 and both["gc_fill"][2] == (5 << 16 | 2)
    assert CASES["graph/inconsistent-self-last-wavefront"].n == 130   # state 129: the second and last lane of the last wavefront


def test_the_violation_cases_hold_what_they_are_named_for():
    base = M.empty_bins()
    VB = X.VIOL_BINS

    def run(name, stored, expanded=True, flags=0):
        return M.violations_model(CASES[f"violations/{name}"], stored, expanded, flags, base)
    mixed = run("mixed-cells", False)
    assert sum(1 for b in range(32) if mixed[b]) >= 5 and sum(1 for b in range(32) if mixed[VB + b]) >= 5
    three = run("three-workgroups", True)
    assert three[6] == 3 and three[2 * VB + 6] == 9 and three[9] == 2 and three[2 * VB + 9] == 520   # invariant 9: the last workgroup alone
    assert three[VB + 6] == 3 and three[VB + 9] == 2 and three[2 * VB + VB + 9] == M.viol_key(577, 0, 1, 9)
    lane = run("one-lane-63", True)
    assert lane[3] == 5 == lane[VB + 3] and lane[2 * VB + 3] == 63 and int(lane[:2 * VB].sum()) == 10
    behind = run("assert-behind", False)
    assert behind[VB + M.BIN_FATAL] == 2 and behind[2 * VB + VB + M.BIN_FATAL] == M.viol_key(400, 1, 2, 0) > behind[2 * VB + VB + 2] == M.viol_key(131, 0, 1, 2)
    assert run("deadlocks", False, flags=M.F_DEADLOCK)[M.BIN_DEADLOCK] > 20 and not run("deadlocks", False)[M.BIN_DEADLOCK]
    init = run("init", False, expanded=False)
    assert [int(init[b]) for b in range(4)] == [6, 5, 5, 6] and not init[VB:2 * VB].any() and run("init", True, expanded=False)[8] == 2
    assert run("step-property", True)[VB + M.BIN_FATAL] == 1 and not run("step-property", False)[VB + M.BIN_FATAL]
    assert not run("step-property-selfloop-only", True)[VB + M.BIN_FATAL]
    # records of all three kinds in the levels of the seeded cases
    c = CASES["graph/level-lo70"]
    kinds = {"none" if p == M.NONE else "valid" if p < i else "bogus" for i, p in enumerate(c.parent.tolist()) if c.hi <= i < c.new_hi}
    assert kinds == {"none", "valid", "bogus"}


def test_the_predicate_case_fails_at_two_states_and_two_indices():
    c = CASES["graph/predicates"]
    fails = {(i, k) for i, s in enumerate(c.states) for k in range(32) if s.fail >> k & 1}
    assert fails == {(5, 9), (530, 3), (531, 2)} and graph_want("graph/predicates")["pred_bad"] == (5 << 8 | 9)


def test_source_and_destination_stand_at_different_labels_on_every_edge():
    c, g = CASES["graph/labels"], graph_want("graph/labels")
    src = np.repeat(np.arange(c.n + 1), g["degree"])
    assert g["edges"] == 7 * c.n == len(src)
    for e, i in enumerate(src.tolist()):
        p, to = int(g["proc"][e]), int(g["dst"][e])
        assert c.states[i].labels[max(p, 0)] != c.states[to].labels[max(p, 0)]
        if p >= 0:   # ... and the table tells the two labels apart
            assert g["unit"][e] == c.unit_tab[p * c.nlabels + i % 3] != c.unit_tab[p * c.nlabels + to % 3]
    assert set(g["proc"][:7].tolist()) == {0, 1, 2, -1}
