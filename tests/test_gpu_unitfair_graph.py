"""The checks label by label of the product's state_graph.hip / engine_live.h on graphs that no search of a model
produced (tests/ufrandgraph.py, through the driver of tests/ufgraph.py), against unitfair.decide_units, which shares no code with them
and which tests/test_unitfair_reference.py holds against the definition over every subset — and shows to answer "violated",
"differently from the reading by processes" and "because of a unit in two conjuncts" often enough on exactly these cases.

What this does NOT cover: k_live_unit<S> and the front end's unit map (tests/test_gpu_labelfair.py keeps those)."""
import functools

import numpy as np
import pytest

import sfrandgraph
import sgraph
import strongfair
import ufgraph
import ufrandgraph as R
import unitfair
from testlib import build_mutants, mutant_tree

pytestmark = pytest.mark.gpu
CASES = R.RELABEL_CASES + R.ONION_CASES


@functools.lru_cache(maxsize=None)
def decide_of(case, check):
    ug = R.graph_of(case)
    g = ug.g
    return unitfair.decide_units(ug.uedges, unitfair.masks_of(ug.of_unit), 64, g.ninit, g.bits, R.done_of(g), R.prop_of(*check), ug.weak, ug.strong)


def table_of(ug):
    return ufgraph.fair_units(ug.of_unit, ug.nunits, ug.nconj, ug.weak, ug.strong)


def device(ug, L=None):
    g = ug.g
    return ufgraph.Graph(g.offsets, g.dst, g.proc, ug.unit, g.pred, g.ninit, L=L)


@pytest.fixture(scope="module")
def devices():
    made = {}

    def get(case):
        if case not in made:
            made[case] = device(R.graph_of(case))
        return made[case]
    yield get
    for G in made.values():
        G.close()


def check_trace(ug, want, check, prefix, cycle):
    """a path of the graph from an initial state into ONE final component, then a closed walk inside it that meets every conjunct"""
    g = ug.g
    rows = [[j for _, j in r] for r in g.edges]
    assert prefix and prefix[0] < g.ninit
    for u, v in zip(prefix, prefix[1:]):
        assert v in rows[u]
    entry = prefix[-1]
    if check[0] >= 0:
        assert prefix[prefix.index(want.witness):] == want.path   # along falling distance, the least successor each time
    assert entry in want.root and all(v in want.root for v in cycle)
    if cycle:
        assert cycle[0] == entry and all(u != v for u, v in zip(cycle, cycle[1:] + cycle[:1]))
    wrong = unitfair.cycle_meets_every_conjunct(ug.uedges, unitfair.masks_of(ug.of_unit), 64, ug.weak, ug.strong, cycle, entry)
    assert wrong is None, wrong
    M, S, T = strongfair.sets(R.prop_of(*check), g.bits, g.ninit, R.done_of(g))
    states = cycle or [entry]
    assert any(T[v] for v in states) and all(M[v] for v in states)


def compare(G, case, check, trace=True):
    """one check against decide_units (rank = identity: the graph's numbering is the device's); returns the two infos"""
    ug = R.graph_of(case)
    g = ug.g
    want = decide_of(case, check)
    kind = check[0]
    if kind < 0:
        info, si = G.live_units(table_of(ug))
    else:
        prop = R.prop_of(*check)
        info, si = G.live_check_units(table_of(ug), kind, prop["p"], prop["q"])
    print(R.case_id(case), check, info, si)
    assert info["violated"] == (1 if want.violated else 0)
    assert info["fair_components"] == si["final_components"] == len(want.final)
    assert (si["rounds"], si["closed_states"]) == (want.rounds, want.closed)
    assert si["scc_builds"] == want.rounds - 1
    if kind < 0:
        if want.violated:
            assert info["root"] == want.first_root and info["root_size"] == len(want.root)
        else:
            assert (info["root"], info["root_size"]) == (0, 0)
    else:
        assert (info["mask_states"], info["bad_starts"]) == (want.mask_states, want.bad_starts)
        if want.violated:
            assert info["witness"] == want.witness
            assert info["root"] == min(want.root) and info["root_size"] == len(want.root)
        else:
            assert (info["witness"], info["root"], info["root_size"]) == (0, 0, 0)
    assert G.live_scc_read(0, g.n).tolist() == want.ids      # the refined ids: a closed state is its own
    if want.violated and trace:
        prefix, cycle = G.live_trace(g.level_start)
        check_trace(ug, want, check, prefix, cycle)
    return info, si


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_unit_checks_equal_the_refinement(devices, case):
    G = devices(case)
    for check in R.checks():
        compare(G, case, check)


def test_the_onion_with_plus_label_escapes_takes_d_plus_one_rounds(devices):
    for m, d, top in R.ONION_CASES:
        ug = R.onion(m, d, top)
        info, si = devices((m, d, top)).live_units(table_of(ug))
        assert (info["violated"], si["rounds"], info["root_size"]) == (1, d + 1, m)


# ---------------------------------------------------------------------------------------------------------------- the identity table, and the order of the calls
IDENTITY = [("sparse", 4099, 2, 3, 2, 0.1), ("cycle_chain", 536, 3, 4, 3, 0.1), ("ring_perm", 255, 1, 2, 2, 0.1), (64, 5, False), (2, 3, True)]


def without_seconds(d):
    return {k: v for k, v in d.items() if k != "seconds"}


def identity(g, weak, strong):
    return ufgraph.fair_units([1 << u for u in range(g.nproc)], g.nproc, g.nproc, weak, strong)


@pytest.mark.parametrize("case", IDENTITY, ids=sfrandgraph.case_id)
def test_the_identity_table_equals_the_strong_entry(case):
    """field by field, ids and traces included: one device graph per entry, the same order of checks, the edges' processes as units"""
    g, weak, strong = sfrandgraph.graph_of(case)
    allp = (1 << g.nproc) - 1
    fu = identity(g, weak, strong)
    with ufgraph.Graph(g.offsets, g.dst, g.proc, g.proc, g.pred, g.ninit) as A, ufgraph.Graph(g.offsets, g.dst, g.proc, g.proc, g.pred, g.ninit) as B:
        for kind, p, q in R.checks():
            prop = R.prop_of(kind, p, q)
            if kind < 0:
                (a, sa), (b, sb) = A.live_strong(allp, weak, strong), B.live_units(fu)
                print("measured", sfrandgraph.case_id(case), "Termination: strong entry", a["seconds"], sa, "| unit entry, identity table", b["seconds"], sb)
            else:
                (a, sa), (b, sb) = A.live_check_strong(allp, weak, strong, kind, prop["p"], prop["q"]), B.live_check_units(fu, kind, prop["p"], prop["q"])
            assert without_seconds(a) == without_seconds(b) and without_seconds(sa) == without_seconds(sb), (kind, p, q)
            assert A.live_scc_read(0, g.n).tolist() == B.live_scc_read(0, g.n).tolist()
            if a["violated"]:
                assert A.live_trace(g.level_start) == B.live_trace(g.level_start)


def test_unit_strong_and_weak_checks_do_not_disturb_each_other():
    """a check by units between a weak and a strong one on ONE graph: each reads as if run alone"""
    case = ("cycle_chain", 536, 3, 4, 3, 0.1, "mixed", True)
    ug = R.graph_of(case)
    g, (_, weak, strong) = ug.g, sfrandgraph.escapes(*case[:6])
    allp = (1 << g.nproc) - 1
    checks = [c for c in R.checks() if c[0] >= 0]

    def weak_answers(G, check):
        prop = R.prop_of(*check)
        ci = G.live_check_masked(allp, weak | strong, check[0], prop["p"], prop["q"])
        return without_seconds(ci) | {"scc_builds": 0}, G.live_scc_read(0, g.n).tolist(), G.live_trace(g.level_start) if ci["violated"] else None

    def strong_answers(G, check):
        prop = R.prop_of(*check)
        ci, si = G.live_check_strong(allp, weak, strong, check[0], prop["p"], prop["q"])
        return without_seconds(ci) | {"scc_builds": 0}, without_seconds(si), G.live_scc_read(0, g.n).tolist(), G.live_trace(g.level_start) if ci["violated"] else None

    def unit_answers(G, check):
        prop = R.prop_of(*check)
        ci, si = G.live_check_units(table_of(ug), check[0], prop["p"], prop["q"])
        return without_seconds(ci) | {"scc_builds": 0}, without_seconds(si), G.live_scc_read(0, g.n).tolist(), G.live_trace(g.level_start) if ci["violated"] else None
    with device(ug) as A, device(ug) as B, device(ug) as C, device(ug) as D:
        _, scc = A.scc()
        alone_w = [weak_answers(A, c) for c in checks]
        alone_s = [strong_answers(B, c) for c in checks]
        alone_u = [unit_answers(C, c) for c in checks]
        assert any(u[1]["rounds"] >= 2 for u in alone_u) and any(u != s for u, s in zip(alone_u, alone_s))
        for k, c in enumerate(checks):
            assert unit_answers(D, c) == alone_u[k], c
            assert weak_answers(D, c) == alone_w[k], c
            assert strong_answers(D, c) == alone_s[k], c
            assert unit_answers(D, c) == alone_u[k], c
        t_units = without_seconds(C.live_units(table_of(ug))[0])
        t_weak = without_seconds(A.live_check(allp, weak | strong))
        assert without_seconds(D.live_units(table_of(ug))[0]) == t_units
        assert without_seconds(D.live_check(allp, weak | strong)) == t_weak
        assert without_seconds(D.live_units(table_of(ug))[0]) == t_units
        assert np.array_equal(D.scc_read(0, g.n), scc)


def test_bad_tables_are_refused(devices):
    case = R.RELABEL_CASES[3]
    ug = R.graph_of(case)
    G = devices(case)
    good = (ug.of_unit, ug.nunits, ug.nconj, ug.weak, ug.strong)
    # (the refusals are the product's, live_query.h's, behind the driver's call name: the driver holds no condition of the table)
    bad = [
        ((ug.of_unit, ug.nunits, ug.nconj, ug.weak | ug.strong, ug.strong), "the weak and the strong mask overlap (a conjunct is WF or SF)"),
        ((ug.of_unit, ug.nunits, ug.nconj, ug.weak | 1 << ug.nconj, ug.strong), "a fairness mask names a conjunct beyond nconj"),
        (([m | 1 << ug.nconj if u == 0 else m for u, m in enumerate(ug.of_unit)], ug.nunits, ug.nconj, ug.weak, ug.strong),
         "of_unit[0] names a conjunct beyond nconj"),
        ((ug.of_unit, 128, ug.nconj, ug.weak, ug.strong), "128 units (at most 127)"),                       # counts out of range
        ((ug.of_unit, ug.nunits, 65, ug.weak, ug.strong), "65 conjuncts (at most 64)"),
        ((ug.of_unit, 1, ug.nconj, ug.weak, ug.strong), "names conjuncts for a unit beyond nunits"),        # units beyond nunits
    ]
    assert ug.nconj < 64 and ug.strong
    for args, words in bad:
        with pytest.raises(sgraph.SgError) as e:
            G.live_units(ufgraph.fair_units(*args))
        assert e.value.code == -1   # MC_EBADCFG
        assert str(e.value).startswith("uf_live_units: ") and words in str(e.value), str(e.value)
    G.live_units(ufgraph.fair_units(*good))


# ---------------------------------------------------------------------------------------------------------------- mutants of the new device code
# Three edits, each of which changes a mask or a comparison and never an address, an index, a loop bound or the monotonicity of a
# fixed point (the refinement's rounds are bounded on the host whatever the kernels store): a mutant can only answer wrongly.
#   * the table staged in LDS loses the lowest conjunct of every unit;
#   * a step that leaves the component counts as taken inside it;
#   * en is taken from the masked graph (the property checks alone).
# A mutant is asked for infos and ids only, never for a trace.
MUTANTS = {
    "staged-table-drops-a-conjunct": ("engine_live.h", "tab[threadIdx.x] = of_unit[threadIdx.x];", "tab[threadIdx.x] = of_unit[threadIdx.x] & (of_unit[threadIdx.x] - 1);"),
    "taken-counts-leaving-steps": ("liveness.h", "        if (scc[dst[k]] == mine) t |= c;", "        t |= c;"),
    "en-from-the-masked-graph": ("liveness.h", "        e |= c;   // (the FULL graph's, as in live_state_masked)", "        if (in_m(dst[k])) e |= c;"),
}
MUTANT_CASES = [("ring_perm", 64, 2, 2, 3, 0.1, "mixed", False), ("ring_perm", 64, 2, 2, 1, 0.1, "plus", True), ("cycle_chain", 65, 1, 2, 3, 0.1, "mixed", False)]


@pytest.fixture(scope="module")
def mutants():
    top = ufgraph.SHIM_DIR / "_build" / "mutants"   # (kept between runs: an unchanged mutant stays fresh)

    def build(name):
        return ufgraph.load(ufgraph.build(csrc=mutant_tree(top, name, MUTANTS[name], also=["state_graph.hip"]), out=top / name))
    return build_mutants(MUTANTS, build)


def run_all(L):
    for case in MUTANT_CASES:
        with device(R.graph_of(case), L) as G:
            for check in R.checks():
                compare(G, case, check, trace=False)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_mutant_of_the_new_device_code_is_caught(mutants, name):
    """on three small cases, every check; the unmutated library passes the same comparisons"""
    try:
        run_all(mutants[name])
    except (AssertionError, sgraph.SgError):   # (a refinement that runs into its bound is MC_ESTATE: caught as well)
        pass
    else:
        pytest.fail(f"mutant {name} survives", pytrace=False)
    run_all(None)
