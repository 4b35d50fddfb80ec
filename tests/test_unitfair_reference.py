"""The references of tests/unitfair.py against each other, with no engine code involved: decide_units (the refinement) against
brute_force_units (the definition over every subset) on seeded small graphs of tests/randgraph.py with random unit maps — units in two
conjuncts, units in none —; decide_units under the identity table against strongfair.decide_strong on all of them; and the conditions
on the device tests' case table (tests/ufrandgraph.py), asserted here so that tests/test_gpu_unitfair_graph.py cannot pass vacuously."""
import random

import randgraph
import sfrandgraph
import strongfair
import ufrandgraph as R
import unitfair

FAMILIES = ("sparse", "cycle_chain", "two_level", "ring_perm")


def small_case(rng, k):
    """a randgraph graph of at most 12 states with a random unit map: (uedges, of_unit as sets, nconj, weak, strong, the Graph)"""
    nproc = rng.randrange(1, 5)
    g = randgraph.bfs_numbered(rng.choice(FAMILIES), rng.choice((1, 2, 3, 5, 7, 9, 10, 11, 11, 11)), k, nproc, rng.random() < 0.5, rng.choice((0.1, 0.5, 1.0)))
    assert g.n <= 12
    nconj = rng.randrange(1, 7)
    nlabels = rng.randrange(1, 4)
    # the unit of (instance, label); the label an instance stands at, per state
    unit_of = {(p, l): p * nlabels + l for p in range(g.nproc) for l in range(nlabels)}
    at = [[rng.randrange(nlabels) for _ in range(g.nproc)] for _ in range(g.n)]
    of_unit = []
    for _ in range(g.nproc * nlabels):
        r = rng.random()
        of_unit.append(set() if r < 0.2 else set(rng.sample(range(nconj), min(nconj, 2))) if r < 0.5 else {rng.randrange(nconj)})
    uedges = [[(unit_of[(p, at[i][p])] if p >= 0 else -1, j) for p, j in row] for i, row in enumerate(g.edges)]
    weak = strong = 0
    for c in range(nconj):
        r = rng.random()
        if r < 0.55:
            strong |= 1 << c
        elif r < 0.85:
            weak |= 1 << c
    return uedges, of_unit, nconj, weak, strong, g


def test_the_refinement_equals_the_definition_on_small_graphs():
    rng = random.Random("unitfair-small")
    verdicts, rounds, two, none = [], [], 0, 0
    onions = [(m, d) for m in (1, 2, 3, 4) for d in (1, 2, 3, 4, 5) if m + d + 1 <= 10]
    for k in range(1200):
        if k % 10 == 0:                  # one in ten is a small onion whose escapes are `+` labels: three rounds and more
            ug = R.onion(*onions[k // 10 % len(onions)])
            uedges, of_unit, nconj, weak, strong, g = ug.uedges, unitfair.masks_of(ug.of_unit), 64, ug.weak, ug.strong, ug.g
        else:
            uedges, of_unit, nconj, weak, strong, g = small_case(rng, k)
        done = sfrandgraph.done_of(g)
        prop = R.prop_of(*rng.choice(R.checks()))
        want = unitfair.brute_force_units(uedges, of_unit, nconj, g.ninit, g.bits, done, prop, weak, strong)
        got = unitfair.decide_units(uedges, of_unit, nconj, g.ninit, g.bits, done, prop, weak, strong)
        assert want is not None and got.violated == want, (uedges, of_unit, g.ninit, g.bits, prop, weak, strong)
        verdicts.append(want)
        rounds.append(got.rounds)
        used = {u for row in uedges for u, _ in row if u >= 0}
        two += any(len(of_unit[u]) == 2 for u in used)
        none += any(not of_unit[u] for u in used)
        # the identity table: every unit is its process, conjunct p = process p
        ident = [{p} for p in range(g.nproc)]
        w, s = weak & ((1 << g.nproc) - 1), strong & ((1 << g.nproc) - 1)
        a = unitfair.decide_units(g.edges, ident, g.nproc, g.ninit, g.bits, done, prop, w, s)
        b = strongfair.decide_strong(g.edges, g.en, g.nproc, g.ninit, g.bits, done, prop, w, s)
        assert a == b, (g.edges, prop, w, s)
    print(sum(verdicts), max(rounds), sum(r >= 2 for r in rounds), two, none)
    assert 0.2 * len(verdicts) <= sum(verdicts) <= 0.8 * len(verdicts)
    assert sum(r >= 2 for r in rounds) >= 50 and two >= 300 and none >= 300


def decide(ug, check, of_unit=None, weak=None, strong=None):
    g = ug.g
    table = unitfair.masks_of(ug.of_unit if of_unit is None else of_unit)
    return unitfair.decide_units(ug.uedges, table, 64, g.ninit, g.bits, R.done_of(g), R.prop_of(*check),
                                 ug.weak if weak is None else weak, ug.strong if strong is None else strong)


def test_the_device_case_table_cannot_pass_vacuously():
    """20 - 80 % of the cases are violated; at least 10 % answer differently when every unit is read as its process; at least 10 % hold
    a unit in two conjuncts that decides the verdict (without its own SF conjunct the answer is the other one)"""
    total = violated = by_process = decisive = 0
    for case in R.RELABEL_CASES + R.ONION_CASES:
        ug = R.graph_of(case)
        assert ug.nunits <= 127 and ug.nconj <= 64 and not ug.weak & ug.strong
        plus = sum(1 << k for k in range(64) if any(ug.of_unit[u] >> k & 1 and not ug.no_plus[u] >> k & 1 for u in ug.two_conj_units))
        for check in R.checks():
            v = decide(ug, check)
            total += 1
            violated += v.violated
            by_process += v.violated != decide(ug, check, ug.by_process, strong=ug.strong & ~plus).violated
            decisive += bool(ug.two_conj_units) and v.violated != decide(ug, check, ug.no_plus, strong=ug.strong & ~plus).violated
    print(total, violated / total, by_process / total, decisive / total)
    assert 0.2 <= violated / total <= 0.8 and by_process / total >= 0.1 and decisive / total >= 0.1
    tops = [R.graph_of(c) for c in R.RELABEL_CASES + R.ONION_CASES if c[-1]]
    assert tops and all(ug.nunits == 127 and ug.nconj == 64 for ug in tops)                    # unit 126, conjunct 63
    assert all(126 in {u for row in ug.uedges for u, _ in row} for ug in tops)
    assert any(ug.two_conj_units for ug in tops) and any(ug.none_units for ug in tops)
    sizes = sorted(R.graph_of(c).g.n for c in R.RELABEL_CASES)
    assert {2, 64, 65, 256, 257} <= set(sizes) and sizes[-1] > 2048
    assert max(len(r) for r in R.graph_of(("hub", 1000, 1, 2, 2, 0.1, "mixed", False)).g.edges) >= 5000
    for m, d, top in R.ONION_CASES:                                                            # the escapes are `+` label units: d + 1 rounds
        ug = R.onion(m, d, top)
        v = decide(ug, (-1, -1, -1))
        assert v.violated and v.rounds == d + 1 and len(v.root) == m and len(ug.two_conj_units) == d
