"""The checks under strong fairness of the product's state_graph.hip / engine_live.h on graphs that no search of a
model produced (tests/sfrandgraph.py, through the driver of tests/sfgraph.py), against strongfair.decide_strong, which shares no code
with them and which tests/test_strongfair_reference.py holds against the definition over every subset — and shows to answer
"violated", "differently from weak fairness" and "in a second round" often enough on exactly these cases.

What this does NOT cover: the kernels that build the CSR arrays and the front end (tests/test_gpu_strongfair.py keeps those)."""
import functools

import numpy as np
import pytest

import liveprops
import randgraph
import sfgraph
import sfrandgraph as R
import sgraph
import strongfair
from testlib import build_mutants, mutant_tree

pytestmark = pytest.mark.gpu
CASES = R.ESCAPE_CASES + R.ONION_CASES


@functools.lru_cache(maxsize=None)
def decide_of(case, check, as_weak=False):
    """the reference's answer, computed once; as_weak: the strong processes read as weak ones"""
    g, weak, strong = R.graph_of(case)
    if as_weak:
        weak, strong = weak | strong, 0
    return strongfair.decide_strong(g.edges, g.en, g.nproc, g.ninit, g.bits, R.done_of(g), R.prop_of(*check), weak, strong)


def device(g, L=None):
    return sfgraph.Graph(g.offsets, g.dst, g.proc, g.pred, g.ninit, L=L)


def all_mask(g):
    return (1 << g.nproc) - 1


@pytest.fixture(scope="module")
def devices():
    made = {}

    def get(case):
        if case not in made:
            made[case] = device(R.graph_of(case)[0])
        return made[case]
    yield get
    for G in made.values():
        G.close()


def check_trace(g, want, check, weak, strong, prefix, cycle):
    """a closed walk of graph edges inside ONE final component that meets the rule on its own states"""
    rows = [[j for _, j in r] for r in g.edges]
    assert prefix and prefix[0] < g.ninit
    for u, v in zip(prefix, prefix[1:]):
        assert v in rows[u]
    entry = prefix[-1]
    if check[0] >= 0:
        w = prefix.index(want.witness)
        assert prefix[w:] == want.path                       # along falling distance, the least successor each time
    assert entry in want.root
    assert all(v in want.root for v in cycle)                # never a state the refinement closed
    if cycle:
        assert cycle[0] == entry
        walk = cycle + cycle[:1]
        assert all(v in rows[u] and u != v for u, v in zip(walk, walk[1:]))
    states = cycle or [entry]
    taken = set()
    for a, b in zip(cycle, cycle[1:] + cycle[:1]):
        taken |= {p for p, j in g.edges[a] if p >= 0 and j == b and j != a}
    disabled = set().union(*[set(range(g.nproc)) - g.en[v] for v in states])
    enabled = set().union(*[g.en[v] for v in states])
    W, F = ({p for p in range(g.nproc) if m >> p & 1} for m in (weak, strong))
    assert W <= taken | disabled and F & enabled <= taken, (W, F, taken, disabled, enabled)
    M, S, T = strongfair.sets(R.prop_of(*check), g.bits, g.ninit, R.done_of(g))
    assert any(T[v] for v in states) and all(M[v] for v in states)


def compare(G, case, check, trace=True, as_weak=False):
    """one check against decide_strong (rank = identity: the graph's numbering is the device's); returns the two infos"""
    g, weak, strong = R.graph_of(case)
    if as_weak:
        weak, strong = weak | strong, 0
    want = decide_of(case, check, as_weak)
    kind = check[0]
    if kind < 0:
        info, si = G.live_strong(all_mask(g), weak, strong)
    else:
        prop = R.prop_of(*check)
        info, si = G.live_check_strong(all_mask(g), weak, strong, kind, prop["p"], prop["q"])
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
        check_trace(g, want, check, weak, strong, prefix, cycle)
    return info, si


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_strong_checks_equal_the_refinement(devices, case):
    G = devices(case)
    for check in R.checks():
        compare(G, case, check)


def test_the_onion_takes_d_plus_one_rounds(devices):
    """the rounds are the reference's in the test above; here they are the construction's own: d + 1 and violated, d + 2 and not with
    the closing process (m >= 2: a core of one state is gone with the state the closing process leaves)"""
    for m, d, closing in R.ONION_CASES:
        g, weak, strong = R.onion(m, d, closing)
        info, si = devices((m, d, closing)).live_strong(all_mask(g), weak, strong)
        print("onion", m, d, closing, info, si, "| the same graph, every process weak:", devices((m, d, closing)).live_check(all_mask(g), weak | strong))
        if not closing:
            assert (info["violated"], si["rounds"]) == (1, d + 1) and info["root_size"] == m
        elif m >= 2:
            assert (info["violated"], si["rounds"]) == (0, d + 2)
    g, weak, strong = R.onion(257, 62, False)
    assert strong >> 63 & 1                                  # process 63, and a bound of 63 rounds, are met


# ---------------------------------------------------------------------------------------------------------------- strong_mask = 0, and the order of the calls
PLAIN = [("sparse", 257, 2, 3, True, 0.1), ("cycle_chain", 268, 2, 3, True, 0.1), ("ring_perm", 65, 1, 3, True, 0.1)]


def without_seconds(d):
    return {k: v for k, v in d.items() if k != "seconds"}


@pytest.mark.parametrize("case", PLAIN, ids=randgraph.case_id)
def test_no_strong_process_equals_the_weak_entry(case):
    """field by field, scc_builds included: one device graph per entry, the same order of checks"""
    g = randgraph.bfs_numbered(*case)
    with device(g) as A, device(g) as B:
        for fair in randgraph.fair_masks(case):
            a, (b, si) = A.live_check(all_mask(g), fair), B.live_strong(all_mask(g), fair, 0)
            assert without_seconds(a) == without_seconds(b) and si["rounds"] == 1 and si["scc_builds"] == 0
            if a["violated"]:
                assert A.live_trace(g.level_start) == B.live_trace(g.level_start)
        for kind, p, q, fair in randgraph.prop_checks(case):
            prop = randgraph.prop_of(kind, p, q)
            a = A.live_check_masked(all_mask(g), fair, kind, prop["p"], prop["q"])
            b, si = B.live_check_strong(all_mask(g), fair, 0, kind, prop["p"], prop["q"])
            assert without_seconds(a) == without_seconds(b), (kind, p, q, fair)
            assert si["rounds"] == 1 and si["scc_builds"] == 0 and si["final_components"] == a["fair_components"]
            # the refined ids of a weak rule: the violating components keep their ids, every other state is its own
            want = liveprops.decide(g.edges, g.en, g.nproc, g.ninit, g.bits, prop, fair)
            ids = list(range(g.n))
            for c in want.violating:
                for v in c:
                    ids[v] = min(c)
            assert B.live_scc_read(0, g.n).tolist() == ids
            if a["violated"]:
                assert A.live_trace(g.level_start) == B.live_trace(g.level_start)


def test_weak_and_strong_checks_do_not_disturb_each_other():
    """a weak check after a strong one, and the reverse, read as if run alone: infos, components, traces, mc_engine_scc_read's array"""
    case = ("cycle_chain", 536, 3, 4, 3, 0.1)
    g, weak, strong = R.graph_of(case)
    both = weak | strong
    checks = [c for c in R.checks() if c[0] >= 0]

    def weak_answers(G, check):
        prop = R.prop_of(*check)
        ci = G.live_check_masked(all_mask(g), both, check[0], prop["p"], prop["q"])
        return without_seconds(ci), G.live_scc_read(0, g.n).tolist(), G.live_trace(g.level_start) if ci["violated"] else None

    def strong_answers(G, check):
        prop = R.prop_of(*check)
        ci, si = G.live_check_strong(all_mask(g), weak, strong, check[0], prop["p"], prop["q"])
        return without_seconds(ci), without_seconds(si), G.live_scc_read(0, g.n).tolist(), G.live_trace(g.level_start) if ci["violated"] else None
    with device(g) as A, device(g) as B, device(g) as C:
        _, scc = A.scc()
        B.scc()
        C.scc()
        alone_w = [weak_answers(A, c) for c in checks]
        alone_s = [strong_answers(B, c) for c in checks]
        assert any(s[1]["rounds"] >= 2 for s in alone_s)
        for k, c in enumerate(checks):                       # interleaved on one graph: the masks' builds are shared, in the same order
            w, s = weak_answers(C, c), strong_answers(C, c)
            assert w == alone_w[k], c
            assert (s[0] | {"scc_builds": 0}, s[1:]) == (alone_s[k][0] | {"scc_builds": 0}, alone_s[k][1:]), c
            assert weak_answers(C, c) == (alone_w[k][0] | {"scc_builds": 0}, *alone_w[k][1:]), c
        assert np.array_equal(C.scc_read(0, g.n), scc)
        t_alone = without_seconds(A.live_check(all_mask(g), both))
        C.live_strong(all_mask(g), weak, strong)
        assert without_seconds(C.live_check(all_mask(g), both)) == t_alone
        assert np.array_equal(C.scc_read(0, g.n), scc)


def test_bad_masks_are_refused(devices):
    case = R.ESCAPE_CASES[3]
    g, weak, strong = R.graph_of(case)
    # (the refusals are the product's, live_query.h's, behind the driver's call name: the driver holds no condition of its own)
    for w, s, words in ((weak | 1 << g.nproc - 1, strong, "the weak and the strong mask overlap (a strongly fair process is weakly fair already)"),
                        (weak, strong | 1 << g.nproc, "a fairness mask names a process instance the program does not have")):
        with pytest.raises(sgraph.SgError) as e:
            devices(case).live_strong(all_mask(g), w, s)
        assert e.value.code == -1   # MC_EBADCFG
        assert str(e.value).startswith("sf_live_strong: " + words), str(e.value)


# ---------------------------------------------------------------------------------------------------------------- mutants of the new kernels
# Three edits of engine_live.h, each of which changes a stored value or a counter and never an address, an index, a loop bound or the
# monotonicity of a fixed point (the refinement's rounds are bounded on the host whatever the kernels store):
#   * k_live_refine judges a blocked component's state by the complement of its en mask: the unblocked states are closed;
#   * k_live_refine reads the component's taken mask where it reads enabled: no component is ever blocked;
#   * k_live_classify counts the open components that are NOT final (first_root stays a root below n).
# A mutant is asked for infos and ids only, never for a trace.
MUTANTS = {
    "refine-closes-the-unblocked": ("live_blockers(all, strong, en_c, tk), en);", "live_blockers(all, strong, en_c, tk), ~en);"),
    "enabled-is-taken": ("const uint64_t tk = taken[c], en_c = enabled[c], o = offsets[v];", "const uint64_t tk = taken[c], en_c = taken[c], o = offsets[v];"),
    "final-counts-the-closed": ("const bool bad = root && live_violates_strong(", "const bool bad = root && !live_violates_strong("),
}


@pytest.fixture(scope="module")
def mutants():
    top = sfgraph.SHIM_DIR / "_build" / "mutants"   # (kept between runs: an unchanged mutant stays fresh)

    def build(name):
        d = mutant_tree(top, name, ("engine_live.h", *MUTANTS[name]), also=["state_graph.hip"])
        return sfgraph.load(sfgraph.build(csrc=d, out=top / name))
    return build_mutants(MUTANTS, build)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_mutant_of_the_new_kernels_is_caught(mutants, name):
    """on the first case and check that need a second round and are violated; the unmutated library passes the same comparison"""
    case, check = next((c, k) for c in R.ESCAPE_CASES for k in R.checks() if decide_of(c, k).rounds >= 2 and decide_of(c, k).violated)
    g = R.graph_of(case)[0]
    with device(g, mutants[name]) as G:
        try:
            compare(G, case, check, trace=False)
        except (AssertionError, sgraph.SgError):   # (a refinement that runs into its bound is MC_ESTATE: caught as well)
            pass
        else:
            pytest.fail(f"mutant {name} survives", pytrace=False)
    with device(g) as G:
        compare(G, case, check, trace=False)
