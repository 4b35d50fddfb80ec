"""The references of tests/strongfair.py against each other, with no engine code involved: decide_strong (the refinement) against
brute_force_strong (the definition over every subset) on seeded small graphs; decide_strong without a strong process against
liveprops.decide on every check of randgraph's LIVE_CASES; and the conditions on the device tests' case table (tests/sfrandgraph.py),
asserted here so that tests/test_gpu_strongfair_graph.py cannot pass vacuously."""
import random

import pytest

import liveprops
import randgraph
import sfrandgraph as R
import strongfair


def small_graph(rng):
    """at most 12 states, up to 5 processes, self loops and parallel edges, Done sinks, three predicate bits; (edges, en, nproc, ninit, bits, done)"""
    n = rng.randrange(1, 13)
    nproc = rng.randrange(1, 5)
    dens = rng.choice((0.8, 1.3, 2.0, 3.0))
    rare = rng.random() < 0.7            # most edges are process 0's, the others are enabled now and then

    def some_process():
        return 0 if rare and rng.random() < 0.7 else rng.randrange(nproc)
    edges = []
    for v in range(n):
        row = []
        if rng.random() < 0.12:
            row.append((-1, v))                                   # a Done state: absorbing
        else:
            while rng.random() < dens / (1 + dens):
                row.append((some_process(), v if rng.random() < 0.08 else rng.randrange(n)))
            if n > 1 and rng.random() < 0.85 and not any(j != v for _, j in row):   # few sinks: a sink that is not Done violates nearly everything
                row.append((some_process(), rng.choice([j for j in range(n) if j != v])))
        edges.append(row)
    ninit = rng.randrange(1, n + 1)
    edges, _, _ = R.bfs_renumber(edges, ninit)   # what the initial states do not reach is dropped: a state graph holds reachable states only
    n = len(edges)
    en = [{p for p, j in edges[v] if p >= 0 and j != v} for v in range(n)]
    bits = [sum(1 << b for b in randgraph.PRED_BITS if rng.random() < 0.4) for _ in range(n)]
    done = [any(p < 0 for p, _ in r) for r in edges]
    return edges, en, nproc, ninit, bits, done


def masks(rng, nproc):
    """disjoint weak / strong masks: every process weak, strong or unfair"""
    weak = strong = 0
    for p in range(nproc):
        r = rng.random() if p else rng.uniform(0.4, 1.0)   # (process 0, which takes most edges, is seldom the strong one)
        if r < 0.5:
            strong |= 1 << p
        elif r < 0.8:
            weak |= 1 << p
    return weak, strong


def test_the_refinement_equals_the_definition_on_small_graphs():
    rng = random.Random("strongfair-small")
    verdicts, rounds, differ = [], [], 0
    onions = [(m, d, c) for m in (1, 2, 3, 4) for d in (1, 2, 3, 4, 5) for c in (False, True) if m + d + 1 <= 10]
    for k in range(1200):
        if k % 10 == 0:                  # one in ten is a small onion: three rounds and more
            g, weak, strong = R.onion(*onions[k // 10 % len(onions)])
            edges, en, nproc, ninit, bits, done = g.edges, g.en, g.nproc, g.ninit, g.bits, R.done_of(g)
        else:
            edges, en, nproc, ninit, bits, done = small_graph(rng)
            weak, strong = masks(rng, nproc)
        kind, p, q = rng.choice(R.checks())
        prop = R.prop_of(kind, p, q)
        want = strongfair.brute_force_strong(edges, en, nproc, ninit, bits, done, prop, weak, strong)
        got = strongfair.decide_strong(edges, en, nproc, ninit, bits, done, prop, weak, strong)
        assert want is not None and got.violated == want, (edges, ninit, bits, prop, weak, strong)
        verdicts.append(want)
        rounds.append(got.rounds)
        differ += want != strongfair.brute_force_strong(edges, en, nproc, ninit, bits, done, prop, weak | strong, 0)
    # the sample is no formality: both verdicts, several rounds, and cases that weak fairness decides the other way
    print(sum(verdicts), max(rounds), sum(r >= 2 for r in rounds), differ)
    assert 0.2 * len(verdicts) <= sum(verdicts) <= 0.8 * len(verdicts)
    assert sum(r >= 2 for r in rounds) >= 100 and max(rounds) >= 3 and differ >= 40


@pytest.mark.parametrize("case", randgraph.LIVE_CASES, ids=randgraph.case_id)
def test_without_a_strong_process_it_is_the_weak_rule(case):
    g = randgraph.bfs_numbered(*case)
    done = R.done_of(g)
    for kind, p, q, fair in randgraph.prop_checks(case):
        prop = randgraph.prop_of(kind, p, q)
        a = liveprops.decide(g.edges, g.en, g.nproc, g.ninit, g.bits, prop, fair)
        b = strongfair.decide_strong(g.edges, g.en, g.nproc, g.ninit, g.bits, done, prop, fair, 0)
        assert (a.violated, a.violating, a.witness, a.path, a.root, a.mask_states, a.bad_starts) == \
               (b.violated, b.final, b.witness, b.path, b.root, b.mask_states, b.bad_starts), (kind, p, q, fair)
        assert b.rounds == 1
    for fair in randgraph.fair_masks(case):   # Termination: randgraph's rule over Tarjan's components
        import livegraph
        comp = livegraph.tarjan(g.n, lambda v: [j for _, j in g.edges[v]])
        bad, root = randgraph.termination(g, comp, fair)
        b = strongfair.decide_strong(g.edges, g.en, g.nproc, g.ninit, g.bits, done, R.prop_of(-1, -1, -1), fair, 0)
        assert (b.violated, b.final, b.first_root) == (bool(bad), {frozenset(m) for m in bad.values()}, root)


def test_the_device_case_table_cannot_pass_vacuously():
    """between 20 % and 80 % of the cases answer "violated", at least 10 % answer differently from the same case with F read as weak,
    at least 25 % need a second round; the onion takes its d + 1 rounds (d + 2 with the closing process and a core of two states or more)"""
    total = violated = differ = second = 0
    for case in R.ESCAPE_CASES + R.ONION_CASES:
        g, weak, strong = R.graph_of(case)
        done = R.done_of(g)
        assert not weak & strong and (weak | strong) < 1 << g.nproc <= 1 << 64
        for check in R.checks():
            prop = R.prop_of(*check)
            v = strongfair.decide_strong(g.edges, g.en, g.nproc, g.ninit, g.bits, done, prop, weak, strong)
            w = strongfair.decide_strong(g.edges, g.en, g.nproc, g.ninit, g.bits, done, prop, weak | strong, 0)
            total += 1
            violated += v.violated
            differ += v.violated != w.violated
            second += v.rounds >= 2
    print(total, violated / total, differ / total, second / total)
    assert 0.2 <= violated / total <= 0.8 and differ / total >= 0.1 and second / total >= 0.25
    sizes = sorted(R.graph_of(c)[0].n for c in R.ESCAPE_CASES)
    assert {1 + 1, 63, 64, 65, 255, 256, 257, 1001} <= set(sizes) and sizes[-1] > 2048
    assert max(len(r) for r in R.graph_of(("hub", 1000, 1, 2, 2, 0.1))[0].edges) >= 5000
    for m, d, closing in R.ONION_CASES:
        g, weak, strong = R.onion(m, d, closing)
        v = strongfair.decide_strong(g.edges, g.en, g.nproc, g.ninit, g.bits, R.done_of(g), R.prop_of(-1, -1, -1), weak, strong)
        if not closing:
            assert v.violated and v.rounds == d + 1 and len(v.root) == m
        elif m >= 2:
            assert not v.violated and v.rounds == d + 2
    assert R.onion(257, 62)[2] >> 63 & 1 and R.onion(257, 62, True)[0].nproc == 64
