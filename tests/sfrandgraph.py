"""Seeded graphs for the checks under strong fairness (tests/sfgraph.py on the device, tests/strongfair.decide_strong beside it), in
tests/randgraph.py's two forms at once.  numpy and `random` alone; nothing of the engine.

escapes   a randgraph.bfs_numbered graph (no escape of its own) with INTERMITTENT STRONG ESCAPES: one to three more processes, each with
          an edge to one added Done state D from a random share of the states (2 - 30 %); every sink that is not Done gets one.  D has
          all predicate bits set, so it decides no check.  The plain processes are weak, the escapes strong: a component is blocked
          where an escape is enabled, and what the refinement leaves of it is decided in a second round.
onion     a core ring of m states of weak process 0; states a_1 .. a_d on detours core[0] -> a_k -> core[1]; strong process 1 has its
          only edge from a_1 to D, strong process k its only edge from a_k to a_(k-1).  Round k closes a_k alone: d + 1 rounds, and the
          core is a fair suffix (violated).  `closing`: one more strong process steps from core[0] to a_d; the core is then blocked in
          round d + 1 and nothing is left after round d + 2 (holds).  The detours are steps of an unfair process of their own while
          64 processes have room for one, else of process 0.

Every graph is searched breadth-first from its initial states once more, rows in order, so that level_start is what a finished search
hands the counterexample builder."""
import functools
import random

import numpy as np

import randgraph

Graph = randgraph.Graph   # name n offsets dst proc pred ninit level_start edges en bits nproc
ALL_BITS = sum(1 << b for b in randgraph.PRED_BITS)


def bfs_renumber(rows, ninit):
    """rows[v] = [(process, successor)] with the initial states first; returns (edges renumbered by discovery, level_start, number)"""
    order, number, level_start = list(range(ninit)), {v: v for v in range(ninit)}, [0]
    lo = 0
    while lo < len(order):
        hi = len(order)
        for v in order[lo:hi]:
            for _, j in rows[v]:
                if j not in number:
                    number[j] = len(order)
                    order.append(j)
        if len(order) > hi:
            level_start.append(hi)
        lo = hi
    return [[(p, number[j]) for p, j in rows[v]] for v in order], level_start, number


def finish(name, rows, ninit, bits_of, nproc):
    edges, level_start, number = bfs_renumber(rows, ninit)
    m = len(edges)
    bits = [0] * m
    for v, i in number.items():
        bits[i] = bits_of(v)
    en = [{p for p, j in edges[i] if p >= 0 and j != i} for i in range(m)]
    offsets, dst = randgraph.csr([[j for _, j in r] for r in edges])
    proc = np.array([p for r in edges for p, _ in r], dtype=np.int8)
    return Graph(name, m, offsets, dst, proc, np.array(bits, dtype=np.uint32), ninit, level_start, edges, en, bits, nproc)


@functools.lru_cache(maxsize=None)
def escapes(family, n, seed, nproc, nesc, done=0.1):
    """(Graph, weak mask, strong mask)"""
    g = randgraph.bfs_numbered(family, n, seed, nproc, False, done)
    rng = random.Random(f"escapes-{family}-{n}-{seed}-{nproc}-{nesc}")
    D = g.n
    rows = [list(r) for r in g.edges] + [[(-1, D)]]
    share = [rng.uniform(0.02, 0.30) for _ in range(nesc)]
    for v in range(g.n):
        if any(p < 0 for p, _ in rows[v]):
            continue   # a Done state stays absorbing
        sink = not rows[v]
        for k in range(nesc):
            if rng.random() < share[k]:
                rows[v].append((nproc + k, D))
        if sink and not rows[v]:
            rows[v].append((nproc + rng.randrange(nesc), D))
    total = nproc + nesc
    graph = finish(f"{g.name}-esc{nesc}", rows, g.ninit, lambda v: ALL_BITS if v == D else g.bits[v], total)
    return graph, (1 << nproc) - 1, ((1 << nesc) - 1) << nproc


@functools.lru_cache(maxsize=None)
def onion(m, d, closing=False):
    """(Graph, weak mask, strong mask)"""
    nstrong = d + (1 if closing else 0)
    own_detour = 2 + nstrong <= 64
    base = 1 if own_detour else 0          # strong process k has the number base + k
    detour = 1 if own_detour else 0
    nproc = base + nstrong + 1
    assert nproc <= 64
    core = list(range(m))
    a = [None] + [m + k - 1 for k in range(1, d + 1)]   # a[k], k = 1 .. d
    D = m + d
    rows = [[(0, core[(i + 1) % m])] for i in range(m)]
    for k in range(1, d + 1):
        rows[core[0]].append((detour, a[k]))
    if closing:
        rows[core[0]].append((base + d + 1, a[d]))
    for k in range(1, d + 1):
        rows.append([(detour, core[1 % m]), (base + k, D if k == 1 else a[k - 1])])
    rows.append([(-1, D)])

    def bits_of(v):
        return ALL_BITS if v == D else (1 if v == core[0] else 0) | (2 if v == a[1] else 0)
    g = finish(f"onion-{m}-{d}" + ("-closing" if closing else ""), rows, 1, bits_of, nproc)
    strong = sum(1 << (base + k) for k in range(1, nstrong + 1))
    return g, 1, strong


# ---------------------------------------------------------------------------------------------------------------- the case tables
# (family, n, seed, nproc, escapes, done): 1, 2, rings of 63 - 65 and 255 - 257 states (D included), about 1000, one of 4099 (2900 of them
# reached), and hub's row of 5000
ESCAPE_CASES = [
    ("sparse", 1, 1, 1, 1, 0.1), ("sparse", 2, 1, 2, 2, 0.1), ("ring_perm", 62, 1, 2, 1, 0.1), ("ring_perm", 63, 1, 3, 2, 0.1),
    ("ring_perm", 64, 2, 2, 3, 0.1), ("sparse", 64, 1, 3, 2, 0.1), ("cycle_chain", 65, 1, 2, 3, 0.1), ("ring_perm", 254, 2, 3, 1, 0.1),
    ("ring_perm", 255, 1, 2, 2, 0.1), ("ring_perm", 256, 3, 2, 1, 0.1), ("sparse", 256, 3, 61, 3, 0.1), ("two_level", 257, 1, 3, 2, 1.0),
    ("sparse", 1000, 1, 3, 2, 0.1), ("ring_perm", 1000, 3, 2, 1, 0.1), ("cycle_chain", 536, 3, 4, 3, 0.1), ("two_level", 1000, 2, 2, 1, 0.1),
    ("sparse", 4099, 2, 3, 2, 0.1), ("hub", 1000, 1, 2, 2, 0.1), ("cycle_chain", 268, 2, 1, 1, 0.1), ("sparse", 257, 5, 2, 1, 1.0),
]
# (m, d, closing)
ONION_CASES = [(1, 1, False), (2, 3, False), (64, 5, False), (257, 62, False), (1, 1, True), (2, 3, True), (64, 5, True), (257, 62, True)]


def case_id(case):
    return "-".join(str(x) for x in case)


def graph_of(case):
    return onion(*case) if len(case) == 3 else escapes(*case)


def checks():
    """the checks asked of every graph: Termination (kind -1), then every kind with every (P, Q) of randgraph.PQ"""
    return [(-1, -1, -1)] + [(kind, p, q) for kind in randgraph.KINDS for p, q in randgraph.PQ]


def prop_of(kind, p, q):
    return {"kind": -1, "p": -1, "q": -1} if kind < 0 else randgraph.prop_of(kind, p, q)


def done_of(g):
    return [any(p < 0 for p, _ in r) for r in g.edges]
