"""The side passes that are templated on a lowering — the CSR build with k_live_proc / k_live_unit / k_live_pred (engine_graph.h), the
coverage histograms (engine_coverage.h) and the -continue passes (engine_violations.h) — against tests/sidemodel.py, on rows of the
table lowering (tests/_sideshim/spec_table.h) that no search produced, launched through tests/sideshim.py in the engine's chunks.  Every
comparison is exact and covers the whole output: what a kernel must not write holds its pre-fill, and the guard zones around every
written buffer are intact.  Every case goes through all three drivers (a case is a level: rows, a seen-set, trace records, ranges).
tests/test_sidepass_reference.py checks the model against the product's host loops and that the cases hold what their names say.  At the
end: five edits of the device headers, each caught by a test here that the product passes."""
import functools

import numpy as np
import pytest

import sidemodel as M
import sideshim as X
from testlib import build_mutants, mutant_tree, survives

pytestmark = pytest.mark.gpu

CASES = M.cases()
VB = X.VIOL_BINS
GRAPH_KEYS = ("slot_index", "degree", "offsets", "dst", "act", "proc", "unit", "pred", "gc_degree", "gc_fill")


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.flatnonzero(got != want)
    assert not len(bad), f"{what}: {len(bad)} differ, the first at {bad[0]}: {int(got[bad[0]]):#x}, expected {int(want[bad[0]]):#x}"


@functools.lru_cache(maxsize=None)
def graph_want(name):
    return M.graph_model(CASES[name])


def check_graph(name, L=None, host=False):
    c, want = CASES[name], graph_want(name)
    got = X.graph(c.prm, c.rows(), c.expanded, c.table, c.nbuckets, c.sparse, c.chunk, c.unit_tab, c.nlabels, c.npred, c.cap, L=L, host=host)
    assert got["edges"] == want["edges"], f"{name}: edges"
    for key in GRAPH_KEYS:
        same(got[key], want[key], f"{name}: {key}")
    assert got["pred_bad"] == want["pred_bad"], f"{name}: the predicates' first_bad"
    assert got["intact"], name
    return got


def coverage_base(c):
    return np.random.default_rng(c.n).integers(0, 1 << 40, size=2 * c.prm.nbins).astype(np.uint64)


def check_coverage(name, L=None, host=False):
    c = CASES[name]
    base = coverage_base(c)
    want, valid = M.coverage_model(c, base)
    got, intact = X.coverage(c.prm, c.rows(), c.parent, c.pslot, c.lo, c.hi, c.hi, c.new_hi, c.chunk, base, L=L, host=host)
    same(got, want, f"{name}: the bins")
    assert int((got - base)[c.prm.nbins:].sum()) == valid, f"{name}: the distinct bins sum to the records that count"
    assert intact, name
    return got - base


def violations_base():
    base = M.empty_bins()   # a table that a level before has written: counts to add to, a minimum that stays, one that does not
    base[3], base[2 * VB + 3], base[VB + 2], base[2 * VB + VB + 2] = 5, 1, 7, M.ALL - 1
    return base


VARIANTS = [(stored, expanded, flags) for stored in (False, True) for expanded in (True, False) for flags in (0, M.F_DEADLOCK)]


def check_violations(name, variants=VARIANTS, L=None, host=False):
    c, base, out = CASES[name], violations_base(), {}
    for stored, expanded, flags in variants:
        what = f"{name}: {'SpecTabStored' if stored else 'SpecTab'}, expanded {expanded}, flags {flags}"
        want = M.violations_model(c, stored, expanded, flags, base)
        got, intact = X.violations(stored, c.prm, c.rows(), c.parent, c.pslot, c.lo, c.hi, c.new_hi, expanded, flags, c.chunk, base, L=L, host=host)
        same(got, want, what)
        assert intact, what
        out[stored, expanded, flags] = got
    return out


# ------------------------------------------------------------------------------------------------------------------- every case, each driver
@pytest.mark.parametrize("name", list(CASES))
def test_graph(name):
    check_graph(name)


@pytest.mark.parametrize("name", list(CASES))
def test_coverage(name):
    check_coverage(name)


@pytest.mark.parametrize("name", list(CASES))
def test_violations(name):
    check_violations(name)


# ------------------------------------------------------------------------------------------------ what a named case is there to show
def test_a_lost_state_and_a_lost_successor_are_counted_with_the_least_key():
    for what, counter in (("self", 0), ("absent", 1), ("no-index", 1)):
        both, alone = check_graph(f"graph/inconsistent-{what}-both"), check_graph(f"graph/inconsistent-{what}-last-wavefront")
        assert both["gc_fill"][counter] >= 2 and alone["gc_fill"][counter] >= 1
        assert both["gc_fill"][2] >> 16 == 5 and alone["gc_fill"][2] >> 16 == 129   # the LOWER index of the two; the last wavefront's only one
        if what == "no-index":   # the degree pass cannot see it
            assert both["gc_degree"][1] == 0 and both["gc_degree"][2] == M.ALL and (both["dst"] == M.NONE).sum() == 2


def test_key_zero_is_nobodys():
    for name in CASES:
        if name.startswith("graph/chain-"):
            got = check_graph(name)
            assert got["gc_degree"][1] == 1 and got["gc_degree"][2] == (3 << 16 | 1)


def test_an_id_beyond_the_bins_and_a_record_that_cannot_be_one_are_counted_nowhere():
    for nbins in (2, 7, X.COV_MAX_BINS):
        c = CASES[f"coverage/ids-nbins{nbins}"]
        added = check_coverage(f"coverage/ids-nbins{nbins}")
        pairs = sum(s.nslots for s in c.states[c.lo:c.hi])
        assert 0 < int(added[:nbins].sum()) < pairs and 0 < int(added[nbins:].sum()) < c.new_hi - c.hi


def test_an_assert_behind_an_invariant_violator_is_in_the_fatal_cell():
    for stored in (False, True):
        got = check_violations("violations/assert-behind", [(stored, True, 0)])[stored, True, 0]
        assert got[VB + M.BIN_FATAL] == 2 and got[2 * VB + VB + M.BIN_FATAL] == M.viol_key(400, 1, 2, 0)
        assert got[VB + 2] - violations_base()[VB + 2] == 1   # ... and the violator in front of it is counted as ever


def test_deadlocks_count_only_when_they_are_checked():
    got = check_violations("violations/deadlocks", [(False, True, 0), (False, True, M.F_DEADLOCK)])
    assert got[False, True, 0][M.BIN_DEADLOCK] == 0 and got[False, True, M.F_DEADLOCK][M.BIN_DEADLOCK] > 20
    assert got[False, True, M.F_DEADLOCK][2 * VB + M.BIN_DEADLOCK] == 63   # lo itself: 63 = 7 * 9


def test_a_flagged_step_is_fatal_only_for_a_lowering_that_checks_stored_states():
    fatal = VB + M.BIN_FATAL
    got = check_violations("violations/step-property", [(False, True, 0), (True, True, 0)])
    assert got[False, True, 0][fatal] == 0
    assert got[True, True, 0][fatal] == 1 and got[True, True, 0][2 * VB + fatal] == M.viol_key(200, 0, 1, 4)
    got = check_violations("violations/step-property-selfloop-only", [(True, True, 0)])
    assert got[True, True, 0][fatal] == 0


def test_the_first_failing_predicate_is_the_least_state_and_index():
    got = check_graph("graph/predicates")
    assert got["pred_bad"] == (5 << 8 | 9)
    assert not got["pred"][5] >> 9 & 1 and not got["pred"][530] >> 3 & 1 and not got["pred"][531] >> 2 & 1


# ---------------------------------------------------------------------------------------------------------------- mutants of the device code
# Five edits of the device headers.  Each changes a count, a key or a lane's activity; none changes an index into a buffer:
#   * cov_bump always takes the uniform path: the lead lane adds every lane's count to ITS bin (a bin cov_bump has range-checked);
#   * viol_note's uniform path offers the key of every lane, counted or not, to the minimum.  (The edit the issue words — the lead lane's
#     key in wave_min_u64's place — is no mutant of these kernels: a wavefront's lanes hold rising state indices, every key rises with
#     the index, and the lead lane is the lowest counted one, so its key IS the minimum.  This is the nearest edit of the same line that
#     changes a result.)
#   * k_coverage_generated's column test loses idx >= lo: the states between the 64-aligned base and lo, rows of the same arena block,
#     are counted once more;
#   * graph_walk<FILL> does not count a destination without an arena index as missing (the edge is written as before);
#   * k_graph_index keeps the LARGEST bad key: ~0, "none", survives.
MUTANTS = {
    "cov-always-uniform": ("engine_coverage.h", "if (__ballot(on && bin != bin0) == 0) {", "if (true) {"),
    "viol-unmasked-minimum": ("engine_violations.h", "wave_min_u64(on ? key : ~0ull)", "wave_min_u64(key)"),
    "column-below-lo": ("engine_coverage.h", "const bool active = col < ncols && idx >= lo && idx < hi;", "const bool active = col < ncols && idx < hi;"),
    "no-index-not-missing": ("engine_graph.h", "if (to == GRAPH_NO_INDEX) { ++missing;", "if (false) { ++missing;"),
    "first-bad-maximum": ("engine_graph.h", "atomicMin(&gc->first_bad, graph_bad_key(i, GRAPH_SLOT_SELF))", "atomicMax(&gc->first_bad, graph_bad_key(i, GRAPH_SLOT_SELF))"),
}


@functools.lru_cache(maxsize=None)
def mutant_libraries():
    top = X.SHIM_DIR / "_build" / "mutants"   # (kept between runs: an unchanged mutant stays fresh)
    return build_mutants(MUTANTS, lambda name: X.build(csrc=mutant_tree(top, name, MUTANTS[name]), out=top / name))


@pytest.fixture(scope="module")
def mutants():
    return {name: X.load(so) for name, so in mutant_libraries().items()}


def test_an_always_uniform_bump_is_caught(mutants):
    assert not survives(lambda: check_coverage("coverage/mixed", L=mutants["cov-always-uniform"]))
    check_coverage("coverage/uniform", L=mutants["cov-always-uniform"])   # (where the lanes agree it is the product)
    check_coverage("coverage/mixed")


def test_an_unmasked_minimum_is_caught(mutants):
    assert not survives(lambda: check_violations("violations/assert-behind", [(False, True, 0)], L=mutants["viol-unmasked-minimum"]))
    check_violations("violations/assert-behind", [(False, True, 0)])


def test_a_column_below_lo_is_caught(mutants):
    for name in ("coverage/uniform", "graph/level-lo63", "graph/level-lo70"):   # lo = 1, 63, 70
        assert not survives(lambda: check_coverage(name, L=mutants["column-below-lo"])), name
        check_coverage(name)
    check_coverage("graph/level-lo0", L=mutants["column-below-lo"])


def test_an_uncounted_missing_index_is_caught(mutants):
    for where in ("both", "last-wavefront"):
        assert not survives(lambda: check_graph(f"graph/inconsistent-no-index-{where}", L=mutants["no-index-not-missing"])), where
        check_graph(f"graph/inconsistent-no-index-{where}")


def test_a_maximum_for_first_bad_is_caught(mutants):
    assert not survives(lambda: check_graph("graph/inconsistent-self-both", L=mutants["first-bad-maximum"]))
    check_graph("graph/inconsistent-self-both")
