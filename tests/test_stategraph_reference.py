"""What tests/test_gpu_stategraph.py relies on, checked without a GPU: the references it holds the device's components and verdicts
against (livegraph.tarjan, liveprops.decide, randgraph.termination) agree with definitions that take no shortcut through components;
the generators keep their promises; the cases the GPU file runs are balanced — taken from the same table with the same seeds — so that
no verdict can be right by always saying the same; and the driver (tests/sgraph.py) compiles for gfx950 and loads."""
import itertools
import random
from collections import namedtuple

import numpy as np
import pytest

import livegraph
import liveprops
import randgraph as R


def comp_of(g):
    return livegraph.tarjan(g.n, lambda v: [j for _, j in g.edges[v]])


def closure(n, adj):
    """reach[u][v]: a path of zero or more edges from u to v (Warshall)"""
    reach = [[u == v or v in adj[u] for v in range(n)] for u in range(n)]
    for k in range(n):
        for u in range(n):
            if reach[u][k]:
                ru, rk = reach[u], reach[k]
                for v in range(n):
                    if rk[v]:
                        ru[v] = True
    return reach


def test_tarjan_is_mutual_reachability():
    rng = random.Random(20)
    nontrivial = 0
    for case in range(300):
        n = rng.randint(1, 12)
        adj = (R.sparse if case % 3 else R.cycle_chain)(n, rng)
        adj = R.shuffled(adj + [[] for _ in range(n - len(adj))], rng)
        reach = closure(n, adj)
        want = [min(u for u in range(n) if reach[v][u] and reach[u][v]) for v in range(n)]
        assert livegraph.tarjan(n, lambda v: adj[v]) == want, adj
        nontrivial += len(set(want)) < n
    assert nontrivial > 100   # (the comparison is not one of singletons)


Small = namedtuple("Small", "edges en bits init nproc")   # what liveprops.brute_force reads of a graph


def small_graphs(seed, count):
    rng = random.Random(seed)
    for k in range(count):
        family = ("sparse", "cycle_chain")[k % 2]
        yield R.bfs_numbered(family, rng.randint(2, 12), rng.randrange(10 ** 6), rng.choice((1, 2, 3)), rng.random() < 0.4, rng.choice((0.1, 1.0)))


@pytest.mark.parametrize("part", range(4))
def test_decide_equals_the_definition(part):
    """liveprops.decide(...).violated against liveprops.brute_force on 4 x 300 (graph, kind, fair mask, p, q) cases"""
    rng = random.Random(100 + part)
    seen = {True: 0, False: 0}
    for g in small_graphs(part, 300):
        kind, (p, q), fair = rng.choice(R.KINDS), rng.choice(R.PQ), rng.getrandbits(g.nproc)
        prop = R.prop_of(kind, p, q)
        want = liveprops.brute_force(Small(g.edges, g.en, g.bits, list(range(g.ninit)), g.nproc), prop, fair)
        assert want is not None   # |M| <= BRUTE_CAP
        got = liveprops.decide(g.edges, g.en, g.nproc, g.ninit, g.bits, prop, fair)
        assert got.violated == want, (g.name, g.edges, g.bits, prop, fair)
        seen[want] += 1
    assert min(seen.values()) >= 60, seen


def test_termination_equals_the_definition():
    """randgraph.termination against every non-empty set of states that is one state or strongly connected by its own edges: violated
    iff one of them holds no Done state and is fair by its own taken / disabled sets"""
    rng = random.Random(7)
    seen = {True: 0, False: 0}
    for k in range(300):
        g = R.bfs_numbered(("sparse", "cycle_chain")[k % 2], rng.randint(1, 10), rng.randrange(10 ** 6), rng.choice((1, 2, 3)), rng.random() < 0.7, rng.choice((0.1, 1.0)))
        fair_mask = rng.choice((rng.getrandbits(g.nproc), (1 << g.nproc) - 1))
        fair = {p for p in range(g.nproc) if fair_mask >> p & 1}
        adj = [{j for _, j in row} for row in g.edges]
        rev = [{u for u in range(g.n) if v in adj[u]} for v in range(g.n)]

        def spans(xs, start, nbr):
            seen, todo = {start}, [start]
            while todo:
                for j in nbr[todo.pop()] & xs:
                    if j not in seen:
                        seen.add(j)
                        todo.append(j)
            return len(seen) == len(xs)
        want = False
        for size in range(1, g.n + 1):
            for X in itertools.combinations(range(g.n), size):
                xs = set(X)
                if size > 1 and not (spans(xs, X[0], adj) and spans(xs, X[0], rev)):
                    continue
                if any(p < 0 for v in X for p, _ in g.edges[v]):
                    continue
                taken = {p for v in X for p, j in g.edges[v] if p >= 0 and j != v and j in xs}
                disabled = set().union(*[set(range(g.nproc)) - g.en[v] for v in X])
                want = want or fair <= taken | disabled
        bad, root = R.termination(g, comp_of(g), fair_mask)
        assert bool(bad) == want and (root is None) == (not bad), (g.name, g.edges, fair_mask)
        seen[want] += 1
    assert min(seen.values()) >= 60, seen


# ---------------------------------------------------------------------------------------------------------------- the GPU file's inputs
def test_the_component_cases_hold_large_components():
    few = [c for c in R.SCC_CASES if len(set(comp_of(R.any_numbered(*c)))) < R.any_numbered(*c).n / 2]
    assert len(few) >= 3
    # the families the device's slow paths need are in the table at the sizes that reach them
    assert {("ring_perm", 4099, 1), ("path_reversed", 4099, 1), ("sparse", 4099, 1), ("hub", 1000, 1), ("dense65", 65, 1)} <= set(R.SCC_CASES)
    assert {c[3] for c in R.LIVE_CASES} == {1, 3, 64} and {c[0] for c in R.LIVE_CASES} == {"sparse", "cycle_chain", "two_level", "ring_perm"}


def test_the_termination_cases_are_balanced():
    verdicts = []
    for case in R.LIVE_CASES:
        g = R.bfs_numbered(*case)
        comp = comp_of(g)
        verdicts += [bool(R.termination(g, comp, fair)[0]) for fair in R.fair_masks(case)]
    share = sum(verdicts) / len(verdicts)
    print("Termination: violated in", sum(verdicts), "of", len(verdicts))
    assert 0.25 <= share <= 0.75


def test_the_property_cases_are_balanced():
    by_kind = {k: [] for k in R.KINDS}
    for case in R.LIVE_CASES:
        g = R.bfs_numbered(*case)
        for kind, p, q, fair in R.prop_checks(case):
            by_kind[kind].append(liveprops.decide(g.edges, g.en, g.nproc, g.ninit, g.bits, R.prop_of(kind, p, q), fair).violated)
    for kind, v in by_kind.items():
        print("kind", kind, ": violated in", sum(v), "of", len(v))
    for kind, v in by_kind.items():
        assert 0.25 <= sum(v) / len(v) <= 0.75, kind


def test_the_masks_name_the_last_process():
    for case in R.LIVE_CASES:
        masks = R.fair_masks(case)
        assert masks[0] == 0 and masks[1] == (1 << case[3]) - 1 and masks[2] == 1 << (case[3] - 1) and len(masks) == 5
    assert any(R.fair_masks(c)[2] == 1 << 63 for c in R.LIVE_CASES)
    # ... and the graphs use it, and predicate 31
    for case in R.LIVE_CASES:
        g = R.bfs_numbered(*case)
        if case[3] == 64 and g.n > 60:
            assert 63 in {p for row in g.edges for p, _ in row}
        if g.n > 60:
            assert any(b >> 31 & 1 for b in g.bits) and not all(b >> 31 & 1 for b in g.bits)


# ---------------------------------------------------------------------------------------------------------------- generator invariants
@pytest.mark.parametrize("case", R.LIVE_CASES, ids=R.case_id)
def test_bfs_numbering(case):
    g = R.bfs_numbered(*case)
    off, dst = g.offsets.astype(np.int64), g.dst
    assert off[0] == 0 and off[-1] == len(dst) == len(g.proc) and np.all(np.diff(off) >= 0) and len(off) == g.n + 1 == len(g.pred) + 1
    assert np.all(dst < g.n) and g.proc.min(initial=0) >= -1 and g.proc.max(initial=0) < g.nproc
    assert [dst[off[v]:off[v + 1]].tolist() for v in range(g.n)] == [[j for _, j in row] for row in g.edges]
    assert g.proc.tolist() == [p for row in g.edges for p, _ in row] and g.pred.tolist() == g.bits
    ls = g.level_start
    assert ls[0] == 0 and (g.n == g.ninit or ls[1] == g.ninit) and ls == sorted(set(ls)) and ls[-1] < g.n
    # a discovery order: scanning the rows in order meets the states 0, 1, 2, ... in order, the initial states given
    nxt = g.ninit
    for row in g.edges:
        for _, j in row:
            assert j <= nxt
            nxt += j == nxt
    assert nxt == g.n
    # every non-initial state has an in-edge from the level before its own (and none from an earlier one)
    level = np.searchsorted(ls, np.arange(g.n), side="right") - 1
    first = {}
    for v, row in enumerate(g.edges):
        for _, j in row:
            first.setdefault(j, level[v])
    assert all(first[j] == level[j] - 1 for j in range(g.ninit, g.n))
    for v, row in enumerate(g.edges):   # a Done state is absorbing
        if any(p < 0 for p, _ in row):
            assert row == [(-1, v)]
        assert g.en[v] == {p for p, j in row if p >= 0 and j != v}


@pytest.mark.parametrize("case", R.SCC_CASES, ids=R.case_id)
def test_any_numbering(case):
    g = R.any_numbered(*case)
    off = g.offsets.astype(np.int64)
    assert off[0] == 0 and off[-1] == len(g.dst) and np.all(np.diff(off) >= 0) and len(off) == g.n + 1 and np.all(g.dst < g.n)
    assert g.n == (case[1] if case[0] not in ("cycle_chain", "dense65") else len(g.edges))
    deg = np.diff(off)
    if case[0] == "hub":
        assert deg.max() == 5000 and np.sort(deg)[-2] <= 2 and np.bincount(g.dst).max() >= 5000
    if case[0] == "sparse" and g.n >= 63:
        rows = [g.dst[off[v]:off[v + 1]].tolist() for v in range(g.n)]
        assert any(v in r for v, r in enumerate(rows)) and any(len(set(r)) < len(r) for r in rows) and deg.min() == 0 and deg.max() == 4
    if case[0] == "ring_perm" and g.n > 2:   # shuffled: the ring does not run along the indices
        assert sum(int(g.dst[v]) == (v + 1) % g.n for v in range(g.n)) < g.n / 2 or g.n < 8


def test_the_driver_builds_and_loads():
    """tests/_sgraph/sgraph.hip with the product's state_graph.hip, for gfx950: one hipcc run of about half a minute where the library is
    not there yet.  Loading it needs no device; every entry point the wrappers name resolves."""
    import sgraph
    L = sgraph.load(sgraph.build())
    assert L.sg_last_error() == b""
    for name in ("sg_create", "sg_destroy", "sg_scc", "sg_scc_read", "sg_live_check", "sg_live_check_masked", "sg_live_scc_read", "sg_pred_read",
                 "sg_live_trace", "sg_scan_exclusive_u32_to_u64", "sg_scan_answers_inclusive"):
        assert getattr(L, name)
