"""Seeded graphs with UNITS and CONJUNCTS for the checks label by label (tests/ufgraph.py on the device, tests/unitfair.decide_units
beside it), built on tests/randgraph.py / tests/sfrandgraph.py: a process-labelled graph is read as a program whose instances have
labels with `+` / `-` modifiers.  numpy and `random` alone; nothing of the engine.

relabel   every plain process of an sfrandgraph.escapes graph is an instance, weakly fair, strongly fair or unfair; in every state it
          stands at a label of one of the classes "rest", "-" (the instance's `-` labels: one unit, in no conjunct) or — weakly fair
          instances only — "+" (a unit of its own: in the instance's WF conjunct and in an SF conjunct of its own).  All ESCAPES become
          labels of ONE more weakly fair instance E: the first escape a `+` label, the second a plain label, the third a `+` label again
          (a state with several keeps the first's class: one instance, one label per state).  Read process by process E is weak and
          obliges nobody to leave; label by label its `+` escapes do.  Style "plus": every plain instance is weakly fair and has no `-`
          label, every escape is a `+` label — a state where an instance stands at a `-` label is a fair place to stutter whatever
          else holds, so only these graphs leave the verdict to the `+` labels.
onion     sfrandgraph.onion with every strong process k read as a `+` label of one weakly fair instance: d + 1 rounds as before.

Unit ids and conjunct bits are drawn from all of 0 .. 126 and 0 .. 63; `top` cases hold unit 126 and conjunct 63.
A UnitGraph is the base Graph with unit (per edge, int8), uedges[i] = [(unit or -1, j)], of_unit (masks, 128 of them), nunits, nconj,
weak / strong (conjunct masks), and the two alternative readings the case table's conditions are about:
  by_process   of_unit[u] = the one process-level conjunct of u's instance (0 for an unfair one), with the instance's keyword
  no_plus      the `+` units lose their own SF conjunct"""
import functools
import random
from collections import namedtuple

import numpy as np

import sfrandgraph

UnitGraph = namedtuple("UnitGraph", "g unit uedges of_unit nunits nconj weak strong by_process no_plus two_conj_units none_units")


def _finish(g, inst_class_of_edge, fair_of, plus_classes, seed, top):
    """inst_class_of_edge(i, p, j) -> (instance, class) for every edge with p >= 0; class "rest", "-" or a `+` label's name"""
    rng = random.Random(f"units-{g.name}-{seed}")
    keys = []
    for i, row in enumerate(g.edges):
        for p, j in row:
            if p >= 0:
                k = inst_class_of_edge(i, p, j)
                if k not in keys:
                    keys.append(k)
    insts = sorted({k[0] for k in keys} | set(fair_of))
    ids = rng.sample(range(126), len(keys))
    if top and ids:
        ids[rng.randrange(len(ids))] = 126
    unit_id = dict(zip(keys, ids))
    # conjuncts: one per fair instance, one per `+` label of a weakly fair instance
    want = [("proc", x) for x in insts if fair_of.get(x, 0)] + [("plus", k) for k in keys if fair_of.get(k[0], 0) == 1 and k[1] in plus_classes]
    bits = rng.sample(range(63), len(want))
    if top and bits:
        bits[rng.randrange(len(bits))] = 63
    bit = dict(zip(want, bits))
    of_unit, by_process, no_plus = [0] * 128, [0] * 128, [0] * 128
    weak = strong = 0
    for x in insts:
        if fair_of.get(x, 0) == 1:
            weak |= 1 << bit[("proc", x)]
        elif fair_of.get(x, 0) == 2:
            strong |= 1 << bit[("proc", x)]
    two, none = [], []
    for k in keys:
        x, cls = k
        f = fair_of.get(x, 0)
        base = 1 << bit[("proc", x)] if f and cls != "-" else 0
        u = unit_id[k]
        by_process[u] = 1 << bit[("proc", x)] if f else 0
        no_plus[u] = base
        of_unit[u] = base
        if ("plus", k) in bit:
            of_unit[u] |= 1 << bit[("plus", k)]
            strong |= 1 << bit[("plus", k)]
            two.append(u)
        if not of_unit[u]:
            none.append(u)
    uedges = [[(unit_id[inst_class_of_edge(i, p, j)] if p >= 0 else -1, j) for p, j in row] for i, row in enumerate(g.edges)]
    unit = np.array([u for row in uedges for u, _ in row], dtype=np.int8)
    nunits = max(ids) + 1 if ids else 0
    nconj = max(bits) + 1 if bits else 0
    return UnitGraph(g, unit, uedges, of_unit, nunits, nconj, weak, strong, by_process, no_plus, two, none)


@functools.lru_cache(maxsize=None)
def relabel(family, n, seed, nproc, nesc, done=0.1, style="mixed", top=False):
    g, _, _ = sfrandgraph.escapes(family, n, seed, nproc, nesc, done)
    rng = random.Random(f"relabel-{g.name}-{seed}")
    E = nproc
    plain = style == "plus"   # every plain instance weakly fair and without `-` labels: what is left to decide is the `+` labels'
    fair_of = {p: 1 if plain else rng.choice((1, 1, 1, 1, 2, 0)) for p in range(nproc)}
    fair_of[E] = 1
    esc_class = ["+a", "+b", "+c"] if plain else ["+a", "rest", "+b"]
    # the label class every plain instance stands at, per state
    choices = {p: ["rest"] * 8 + ([] if plain else ["-"]) + (["+x"] if fair_of[p] == 1 else []) for p in range(nproc)}
    at = [{p: rng.choice(choices[p]) for p in range(nproc)} for _ in range(g.n)]

    def of_edge(i, p, j):
        if p < nproc:
            return (p, at[i][p])
        first = min(q for q, _ in g.edges[i] if q >= nproc)
        return (E, esc_class[first - nproc])
    return _finish(g, of_edge, fair_of, {"+a", "+b", "+c", "+x"}, seed, top)


@functools.lru_cache(maxsize=None)
def onion(m, d, top=False):
    g, weak, strong = sfrandgraph.onion(m, d)
    X = 100   # the weakly fair instance whose `+` labels the strong processes become
    strongs = {p for p in range(g.nproc) if strong >> p & 1}

    def of_edge(i, p, j):
        return (X, f"+{p}") if p in strongs else (p, "rest")
    fair_of = {p: 1 if weak >> p & 1 else 0 for p in range(g.nproc) if p not in strongs}
    fair_of[X] = 1
    return _finish(g, of_edge, fair_of, {f"+{p}" for p in strongs}, 0, top)


# (family, n, seed, nproc, escapes, done, style, top): 1 and 2 states, rings around the wavefront and workgroup sizes, one of 4099 raw states,
# hub's row of 5000 edges
RELABEL_CASES = [
    ("sparse", 1, 1, 1, 1, 0.1, "mixed", False), ("sparse", 2, 1, 2, 2, 0.1, "mixed", False), ("ring_perm", 63, 1, 3, 2, 0.1, "mixed", True), ("ring_perm", 64, 2, 2, 3, 0.1, "mixed", False),
    ("cycle_chain", 65, 1, 2, 3, 0.1, "mixed", False), ("ring_perm", 255, 1, 2, 2, 0.1, "mixed", True), ("ring_perm", 256, 3, 2, 1, 0.1, "mixed", False),
    ("two_level", 257, 1, 3, 2, 1.0, "mixed", False), ("cycle_chain", 536, 3, 4, 3, 0.1, "mixed", True), ("sparse", 4099, 2, 3, 2, 0.1, "mixed", True),
    ("ring_perm", 4099, 1, 3, 3, 0.1, "mixed", True), ("hub", 1000, 1, 2, 2, 0.1, "mixed", False),
    ("ring_perm", 63, 1, 1, 2, 0.1, "plus", False), ("ring_perm", 64, 2, 2, 1, 0.1, "plus", True), ("ring_perm", 256, 3, 1, 1, 0.1, "plus", False),
    ("cycle_chain", 268, 2, 1, 2, 0.1, "plus", False), ("ring_perm", 1000, 3, 2, 1, 0.1, "plus", True), ("two_level", 257, 1, 2, 2, 0.1, "plus", False),
]
ONION_CASES = [(2, 3, False), (64, 5, True)]


def case_id(case):
    return "-".join(str(x) for x in case)


def graph_of(case):
    return onion(*case) if len(case) == 3 else relabel(*case)


checks = sfrandgraph.checks
prop_of = sfrandgraph.prop_of
done_of = sfrandgraph.done_of
