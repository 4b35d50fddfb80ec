"""The strongly-connected-components pass, the fairness checks, the counterexample builder and the two device scans of the product's
state_graph.hip / engine_live.h on graphs that no search of a model produced (tests/randgraph.py, through the driver of tests/sgraph.py),
against references that share no code with them: livegraph.tarjan, randgraph.termination (DESIGN section 16 over arrays) and
liveprops.decide (section 17), each of which tests/test_stategraph_reference.py holds against a definition without components — and
which it shows to answer "violated" and "holds" about equally often on exactly these cases.

What this does NOT cover: the kernels that build the CSR arrays from the arena (engine_graph.h, k_live_proc, k_live_pred) and the front
end's classification of properties; the model-based tests (test_gpu_graph, test_gpu_liveness, test_gpu_liveprops) keep those."""
import functools

import numpy as np
import pytest

import livegraph
import liveprops
import randgraph as R
import sgraph
from testlib import build_mutants, mutant_tree, survives

pytestmark = pytest.mark.gpu
ALL_SCC = [("any",) + c for c in R.SCC_CASES] + [("bfs",) + c for c in R.LIVE_CASES]


def graph_of(case):
    return R.any_numbered(*case[1:]) if case[0] == "any" else R.bfs_numbered(*case[1:])


@functools.lru_cache(maxsize=None)
def tarjan_of(case):
    """the reference's component ids of a case of ALL_SCC, computed once and left unchanged"""
    g = graph_of(case)
    a = np.array(livegraph.tarjan(g.n, lambda v: [j for _, j in g.edges[v]]), dtype=np.uint32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def decide_of(case, check):
    g = R.bfs_numbered(*case)
    kind, p, q, fair = check
    return liveprops.decide(g.edges, g.en, g.nproc, g.ninit, g.bits, R.prop_of(kind, p, q), fair)


def device(g, L=None):
    return sgraph.Graph(g.offsets, g.dst, g.proc, g.pred, g.ninit, L=L)


def all_mask(g):
    return (1 << g.nproc) - 1


# ---------------------------------------------------------------------------------------------------------------- components
_scc_infos = {}


def compare_components(G, case):
    g, want = graph_of(case), tarjan_of(case)
    si, scc = G.scc()
    print(R.case_id(case), si)
    assert si["states"] == g.n == len(scc)
    assert np.array_equal(scc, want)                       # ids included: the least index of the component
    sizes = np.bincount(want, minlength=g.n)
    assert (si["components"], si["nontrivial"], si["largest"]) == (int((sizes > 0).sum()), int((sizes > 1).sum()), int(sizes.max()))
    return si, scc


def components_info(case):
    """the mc_scc_info of a case, from the one run of it that compares everything"""
    if case not in _scc_infos:
        g = graph_of(case)
        with device(g) as G:
            si, scc = compare_components(G, case)
            n = g.n
            k, m = n // 3, max(1, n // 2)
            for first, count in ((0, 1), (n - 1, 1), (k, min(m, n - k))):
                assert np.array_equal(G.scc_read(first, count), scc[first:first + count])
            again, scc2 = G.scc()                          # a second build on the same object: the same arrays
            assert np.array_equal(scc, scc2)               # (the numbers of sweeps may differ: how far an in-place sweep carries a value is the scheduler's)
            assert all(again[k] == si[k] for k in ("states", "components", "nontrivial", "largest", "passes"))
        _scc_infos[case] = si
    return _scc_infos[case]


@pytest.mark.parametrize("case", ALL_SCC, ids=R.case_id)
def test_components_equal_tarjans(case):
    components_info(case)


def test_the_slow_paths_of_the_component_search_were_taken():
    """several colouring passes, and fixed points of more than 8 batches of sweeps in each of the three loops, are in the table: asserted
    on the infos of the runs above (a case that has not run yet runs now), so that these paths cannot drop out silently"""
    infos = {c: components_info(c) for c in ALL_SCC}
    many = 8 * sgraph.SCC_BATCH
    assert any(si["passes"] >= 2 for si in infos.values())
    for key in ("trim_rounds", "colour_rounds", "backward_rounds"):
        assert any(si[key] > many for si in infos.values()), key
    slow = [c for c, si in infos.items() if all(si[k] > many for k in ("trim_rounds", "colour_rounds", "backward_rounds"))]
    print("all three loops past", many, "sweeps:", [R.case_id(c) for c in slow])
    assert slow


# ---------------------------------------------------------------------------------------------------------------- Termination
@pytest.fixture(scope="module")
def devices():
    """one device graph per labelled case, shared by the tests below"""
    made = {}

    def get(case):
        if case not in made:
            made[case] = device(R.bfs_numbered(*case))
        return made[case]
    yield get
    for G in made.values():
        G.close()


def check_termination_trace(g, comp, fair_mask, root, prefix, cycle):
    """what tests/test_gpu_liveness.py::test_counterexample demands of an engine's counterexample"""
    rows = [[j for _, j in r] for r in g.edges]
    done = [any(p < 0 for p, _ in r) for r in g.edges]
    fair = {p for p in range(g.nproc) if fair_mask >> p & 1}
    assert prefix and prefix[0] < g.ninit                                   # starts at an initial state
    for u, v in zip(prefix, prefix[1:]):
        assert v in rows[u]                                                 # every step is an edge
    stay = prefix[-1]
    assert comp[stay] == root
    if not cycle:   # stuttering: exactly where every fair process is disabled
        assert not done[stay] and not (fair & g.en[stay])
        return
    assert cycle[0] == stay                                                 # the prefix ends where the cycle starts
    walk = cycle + [cycle[0]]
    for u, v in zip(walk, walk[1:]):
        assert v in rows[u] and u != v                                      # closed, along real edges
    assert all(comp[v] == root for v in cycle)                              # inside the chosen component
    assert not any(done[v] for v in cycle)                                  # no state on it is Done
    taken = set()
    for a, b in zip(cycle, cycle[1:] + cycle[:1]):
        taken |= {p for p, j in g.edges[a] if p >= 0 and j == b and j != a}
    disabled = set()
    for v in cycle:
        disabled |= set(range(g.nproc)) - g.en[v]
    assert fair <= (taken | disabled), (fair, taken, disabled)              # the cycle itself meets the fairness condition


def compare_termination(G, case, fair, trace=True):
    g, comp = R.bfs_numbered(*case), tarjan_of(("bfs",) + case).tolist()
    bad, root = R.termination(g, comp, fair)
    li = G.live_check(all_mask(g), fair)
    print(R.case_id(case), hex(fair), li)
    assert li["violated"] == (1 if bad else 0) and li["fair_components"] == len(bad)
    if bad:
        assert li["root"] == root and li["root_size"] == len(bad[root])     # the least id among the fair components without a Done state
        if trace:
            prefix, cycle = G.live_trace(g.level_start)
            check_termination_trace(g, comp, fair, root, prefix, cycle)
    else:
        assert li["root"] == 0 and li["root_size"] == 0


@pytest.mark.parametrize("case", R.LIVE_CASES, ids=R.case_id)
def test_termination_equals_the_rule(devices, case):
    G = devices(case)
    for fair in R.fair_masks(case):
        compare_termination(G, case, fair)


# ---------------------------------------------------------------------------------------------------------------- property checks
def compare_check(G, case, check, built, trace=True):
    """one check against liveprops.decide (rank = identity: the graph's numbering is the device's).  built: the q whose masked
    components this device graph holds already (<>[]P adds none: that kind uses the full graph's)"""
    g, want = R.bfs_numbered(*case), decide_of(case, check)
    kind, p, q, fair = check
    prop = R.prop_of(kind, p, q)
    ci = G.live_check_masked(all_mask(g), fair, kind, prop["p"], prop["q"])
    print(R.case_id(case), check, ci)
    assert ci["violated"] == (1 if want.violated else 0)
    assert (ci["mask_states"], ci["bad_starts"]) == (want.mask_states, want.bad_starts)
    assert ci["fair_components"] == len(want.violating)   # as test_gpu_liveprops.py: the fair components of G[M] with a T state, reachable or not
    assert ci["scc_builds"] == (0 if kind == liveprops.STABLE or q in built else 1)
    if kind != liveprops.STABLE:
        built.add(q)
    if want.violated:
        assert ci["witness"] == want.witness
        assert ci["root"] == min(want.root) and ci["root_size"] == len(want.root)   # the component Verdict.path ends in
    else:
        assert (ci["witness"], ci["root"], ci["root_size"]) == (0, 0, 0)
    # the components the check judged: Verdict.comp on the states of M, the state itself outside M
    assert G.live_scc_read(0, g.n).tolist() == want.comp
    if want.violated and trace:
        prefix, cycle = G.live_trace(g.level_start)
        assert prefix[0] < g.ninit and want.witness in prefix
        w = prefix.index(want.witness)
        assert prefix[w:] == want.path                                        # along falling distance, the least successor each time
        rows = [[j for _, j in r] for r in g.edges]
        for u, v in zip(prefix, prefix[1:]):
            assert v in rows[u]
        walk = cycle + cycle[:1]
        assert all(v in want.root for v in cycle) and all(v in rows[u] and u != v for u, v in zip(walk, walk[1:]))


@pytest.mark.parametrize("case", R.LIVE_CASES, ids=R.case_id)
def test_property_checks_equal_the_rule(devices, case):
    G = devices(case)
    g = R.bfs_numbered(*case)
    G.scc()                                  # components and everything kept with them built anew: no mask's components are there
    assert np.array_equal(G.pred_read(0, g.n), g.pred)
    built = set()
    for check in R.prop_checks(case):
        compare_check(G, case, check, built)
    # the full graph's components are untouched by the masked builds
    assert np.array_equal(G.scc_read(0, g.n), tarjan_of(("bfs",) + case))


@pytest.mark.parametrize("family", ["path_reversed", "path"])
def test_the_reach_pass_converges_inside_its_bound(family):
    """4099 states in a row, M all of them (<>[]P, P false in the sink alone): the one violating component is the sink, and its distance
    travels the whole path one state per sweep in the worst case — n - 1 sweeps and the batch that sees no change, inside the guard's
    n + SCC_BATCH.  path_reversed: v -> v - 1, the values travel up the indices; path: v -> v + 1, down.  Measured on an MI355X: 4112
    sweeps and 23 ms either way."""
    n = 4099
    g0 = R.any_numbered(family, n, 1)
    sink = 0 if family == "path_reversed" else n - 1
    pred = np.full(n, 1, dtype=np.uint32)
    pred[sink] = 0
    proc = np.zeros(len(g0.dst), dtype=np.int8)
    edges = [[(0, j) for _, j in r] for r in g0.edges]
    en = [{0} if r else set() for r in edges]
    want = liveprops.decide(edges, en, 1, 1, pred.tolist(), R.prop_of(liveprops.STABLE, 0, -1), 1)
    assert want.violated and want.violating == {frozenset([sink])} and want.mask_states == n == want.bad_starts and want.witness == 0
    with sgraph.Graph(g0.offsets, g0.dst, proc, pred, 1) as G:
        ci = G.live_check_masked(1, 1, liveprops.STABLE, 0, -1)
        print(family, ci)
        assert (ci["violated"], ci["fair_components"], ci["mask_states"], ci["bad_starts"], ci["witness"], ci["root"], ci["root_size"], ci["scc_builds"]) == \
               (1, 1, n, n, 0, sink, 1, 0)
        assert G.live_scc_read(0, n).tolist() == want.comp
        if family == "path_reversed":
            assert ci["sweeps"] >= n
        assert ci["sweeps"] <= n + 2 * sgraph.SCC_BATCH   # (the guard lets no batch start past n + SCC_BATCH sweeps)


# ---------------------------------------------------------------------------------------------------------------- the scans
SCAN_SIZES = (1, 2, 255, 256, 257, 65537)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_exclusive_u32_to_u64(n):
    a = np.random.default_rng(n).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    want = np.concatenate(([0], np.cumsum(a.astype(np.uint64), dtype=np.uint64)[:-1])).astype(np.uint64)
    assert np.array_equal(sgraph.scan_exclusive_u32_to_u64(a), want)
    small = (a % 5).astype(np.uint32)         # degrees as a graph has them
    assert np.array_equal(sgraph.scan_exclusive_u32_to_u64(small), np.concatenate(([0], np.cumsum(small.astype(np.uint64), dtype=np.uint64)[:-1])).astype(np.uint64))


def test_scan_offsets_do_not_wrap_past_32_bits():
    a = np.array([0xffffffff] * 3 + [1] * 300, dtype=np.uint32)
    want = np.concatenate(([0], np.cumsum(a.astype(np.uint64), dtype=np.uint64)[:-1])).astype(np.uint64)
    assert int(want[3]) == 3 * 0xffffffff > 2 ** 32 and int(want[-1]) == 3 * 0xffffffff + 299
    assert np.array_equal(sgraph.scan_exclusive_u32_to_u64(a), want)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_answers_inclusive(n):
    rng = np.random.default_rng(n)
    for a in (rng.choice(np.array([0, 1, 7, 255], dtype=np.uint8), size=n), np.zeros(n, dtype=np.uint8), np.full(n, 255, dtype=np.uint8)):
        assert np.array_equal(sgraph.scan_answers_inclusive(a), np.cumsum(a != 0, dtype=np.uint32))


# ---------------------------------------------------------------------------------------------------------------- mutants of the device code
# Three edits of engine_live.h, each of which changes a stored value or a counter and never an address, an index, a loop bound or the
# monotonicity of a fixed point:
#   * k_scc_renumber stores r, a component's largest index, where it stores min(l, r): r < n is checked on that line, and every later
#     reader (k_scc_sizes, k_live_reduce, the reads) only needs scc[v] to be one index per component below n, which r is;
#   * k_scc_stats counts the roots of size > 0 as non-trivial: a counter of LiveCounters alone;
#   * k_live_witness takes every state for initial: more states of M with a distance become bad starts; the witness is still a state of M
#     with a distance, which is all the host's descent along falling distances needs to end in a component.
# A mutant is asked for components, infos and check infos only, never for a trace.
MUTANTS = {
    "renumber-stores-the-root": ("scc[v] = l < r ? l : r;", "scc[v] = r;"),
    "stats-count-every-root": ("big = (unsigned)__popcll(__ballot(sz > 1))", "big = (unsigned)__popcll(__ballot(sz > 0))"),
    "witness-takes-every-state-for-initial": ("live_in_start(ck, bits, v < init_states)", "live_in_start(ck, bits, true)"),
}


@pytest.fixture(scope="module")
def mutants():
    top = sgraph.SHIM_DIR / "_build" / "mutants"   # (kept between runs: an unchanged mutant stays fresh)

    def build(name):
        d = mutant_tree(top, name, ("engine_live.h", *MUTANTS[name]), also=["state_graph.hip"])
        return sgraph.load(sgraph.build(csrc=d, out=top / name))
    return build_mutants(MUTANTS, build)


def test_a_wrong_component_id_is_caught(mutants):
    case = ("any", "cycle_chain", 268, 1)
    with device(graph_of(case), mutants["renumber-stores-the-root"]) as G:
        assert not survives(lambda: compare_components(G, case))
    with device(graph_of(case)) as G:
        compare_components(G, case)


def test_a_wrong_count_of_components_is_caught(mutants):
    case = ("any", "sparse", 65, 1)
    with device(graph_of(case), mutants["stats-count-every-root"]) as G:
        assert not survives(lambda: compare_components(G, case))
    with device(graph_of(case)) as G:
        compare_components(G, case)


def test_a_wrong_set_of_starts_is_caught(mutants):
    """<>Q may only be entered at an initial state: the first check of the table in which another state of M reaches a violating
    component as well"""
    def differs(case, check):
        g = R.bfs_numbered(*case)
        kind, p, q, fair = check
        everywhere = liveprops.decide(g.edges, g.en, g.nproc, g.n, g.bits, R.prop_of(kind, p, q), fair)
        return check[0] == liveprops.EVENTUALLY and everywhere.bad_starts != decide_of(case, check).bad_starts
    case, check = next((c, k) for c in R.LIVE_CASES for k in R.prop_checks(c) if k[0] == liveprops.EVENTUALLY and differs(c, k))
    with device(R.bfs_numbered(*case), mutants["witness-takes-every-state-for-initial"]) as G:
        assert not survives(lambda: compare_check(G, case, check, set(), trace=False))
    with device(R.bfs_numbered(*case)) as G:
        compare_check(G, case, check, set(), trace=False)
