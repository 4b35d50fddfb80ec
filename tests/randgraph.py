"""Seeded graph generators for the tests that drive the product's StateGraph directly (tests/sgraph.py): CSR arrays as mc_engine_graph
would leave them, but of shapes no PlusCal model of this repository produces — several colouring passes with trims between them, fixed
points that run for hundreds of batches against the numbering, rows of 5000 edges beside rows of one, duplicate edges and self loops,
process 63 and predicate 31, components that straddle wavefronts and workgroups.  numpy and `random` alone; nothing of the engine.

A graph comes in two forms at once: offsets / dst / proc / pred (+ ninit, level_start) for the device, and edges[i] = [(process or -1,
j)], en[i] = the processes with a real step in i, bits[i] for tests/liveprops.decide and termination() below.

Numbering.  ANY: the family's own order or a random shuffle of it, unreachable states allowed (components alone are asked of these).
BFS: the family's graph searched breadth-first from `ninit` initial states, rows in order; what is not reached is dropped, the states are
renumbered by discovery and level_start holds the first state of every level — what a finished search hands the counterexample builder.

No family has successors beyond the states (`dst >= n`): engine_graph.h's k_graph_fill does write 0xffffffff for a successor whose key
has no arena index, but it counts that as `missing` in the same breath and Engine::graph_build then fails with "no graph was built"
(graph_inconsistent) and releases the arrays — also after a budget-stopped search, whose unexpanded states simply have empty rows.  No
built graph holds such an entry, so the `dangling` family the kernels' `d < n` guards might suggest is left out on purpose.

Labels (BFS graphs).  Every edge gets a uniformly random process of `nproc`; a Done state is absorbing, its only edge (-1, self), and a
fraction `done` of the sinks is made Done.  `escape`: one more state D, Done, and an edge of the LAST process from every other state to
it — that process is then enabled everywhere and taken inside no component, which is what makes a weakly fair behaviour leave every
cycle: without such graphs nearly every case would be "violated" (any sink that is not Done violates Termination under every mask).
pred: bits 0, 1 and 31, each drawn per state with a density of 0.1, 0.5 or 0.9 (D's with 0.65)."""
import functools
import random
from collections import namedtuple

import numpy as np

Graph = namedtuple("Graph", "name n offsets dst proc pred ninit level_start edges en bits nproc")
KINDS = (0, 1, 2, 3)                       # liveprops: LEADS_TO, INF_OFTEN, EVENTUALLY, STABLE
PQ = ((0, 1), (31, 0), (1, 31))
PRED_BITS = (0, 1, 31)
CHAIN = (1, 2, 3, 63, 64, 65, 70)


# ---------------------------------------------------------------------------------------------------------------- families: adjacency lists
def sparse(n, rng):
    adj = []
    for v in range(n):
        row = []
        for _ in range(rng.randrange(5)):
            r = rng.random()
            if r < 0.3:
                row.append((v + rng.choice((-2, -1, 1, 2))) % n)
            elif r < 0.36:
                row.append(v)                          # a self loop
            elif r < 0.44 and row:
                row.append(rng.choice(row))            # a duplicate edge
            else:
                row.append(rng.randrange(n))
        adj.append(row)
    return adj


def ring(n, rng):
    return [[(v + 1) % n] for v in range(n)]


def path(n, rng):
    return [[v + 1] if v + 1 < n else [] for v in range(n)]


def path_reversed(n, rng):
    return [[v - 1] if v else [] for v in range(n)]


def cycle_chain(n, rng):
    """cycles of CHAIN's sizes (a cycle of one state is a self loop), as many rounds of them as fit n, linked forward by single edges
    from a random state of one to a random state of the next; below one round (the small graphs of the reference's own tests): cycles of
    1, 2, 3, 1, ... states while they fit"""
    sizes = list(CHAIN) * (n // sum(CHAIN))
    while not n // sum(CHAIN) and sum(sizes) + (1, 2, 3)[len(sizes) % 3] <= n:
        sizes.append((1, 2, 3)[len(sizes) % 3])
    adj, first = [], []
    for s in sizes:
        base = len(adj)
        first.append((base, s))
        adj += [[base + (k + 1) % s] for k in range(s)]
    for (a, sa), (b, sb) in zip(first, first[1:]):
        adj[a + rng.randrange(sa)].append(b + rng.randrange(sb))
    return adj


def hub(n, rng):
    """rows of one or two edges, but for state 0 with 5000 out-edges; state 1 has in-degree 5000 (every other row ends there once)"""
    assert n >= 4
    adj = [[1] + ([rng.randrange(n)] if rng.random() < 0.5 else []) for v in range(n)]
    adj[1] = [0, rng.randrange(n)]
    adj[0] = [1] * (5000 - (n - 2)) + [rng.randrange(n) for _ in range(n - 2)]
    rng.shuffle(adj[0])
    assert len(adj[0]) == 5000 and sum(row.count(1) for row in adj) >= 5000
    return adj


def dense65(n, rng):
    return [[u for u in range(65) if u != v] for v in range(65)]


def two_level(n, rng):
    """a ring of n // 2 states, tendrils of n // 8 states leading in and out in turn, and a two-state cycle at the far end of every
    tendril, so that no trim eats a tendril before a colouring pass has taken that cycle: trim and colouring alternate"""
    core = max(2, n // 2)
    adj = [[(v + 1) % core] for v in range(core)]
    left = n - core
    tend = 0
    while left >= 3:
        length = min(left - 2, max(1, n // 8))
        a = len(adj)
        adj += [[a + 1], [a]]                                      # the two-state cycle
        chain = list(range(len(adj), len(adj) + length))
        adj += [[] for _ in chain]
        if tend % 2 == 0:                                          # cycle -> tendril -> core
            adj[a].append(chain[0])
            for x, y in zip(chain, chain[1:]):
                adj[x].append(y)
            adj[chain[-1]].append(rng.randrange(core))
        else:                                                      # core -> tendril -> cycle
            adj[rng.randrange(core)].append(chain[0])
            for x, y in zip(chain, chain[1:]):
                adj[x].append(y)
            adj[chain[-1]].append(a)
        left -= 2 + length
        tend += 1
    adj += [[] for _ in range(left)]
    return adj


FAMILIES = {"sparse": sparse, "ring_perm": ring, "path": path, "path_reversed": path_reversed, "cycle_chain": cycle_chain, "hub": hub,
            "dense65": dense65, "two_level": two_level}
KEEP_ORDER = ("path", "path_reversed", "dense65")   # the family's own numbering is the point


def csr(adj):
    offsets = np.zeros(len(adj) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in adj], dtype=np.uint64)
    dst = np.array([j for r in adj for j in r], dtype=np.uint32)
    return offsets, dst


def shuffled(adj, rng):
    n = len(adj)
    new = list(range(n))
    rng.shuffle(new)                       # new[v]: the index state v gets
    out = [None] * n
    for v, row in enumerate(adj):
        out[new[v]] = [new[j] for j in row]
    return out


@functools.lru_cache(maxsize=None)
def any_numbered(family, n, seed):
    """a Graph with offsets / dst alone (and edges[i] = [(0, j)]): for the component cases"""
    rng = random.Random(f"{family}-{n}-{seed}")
    adj = FAMILIES[family](n, rng)
    if family not in KEEP_ORDER:
        adj = shuffled(adj, rng)
    offsets, dst = csr(adj)
    return Graph(f"{family}-{n}", len(adj), offsets, dst, None, None, 0, None, [[(0, j) for j in r] for r in adj], None, None, 0)


@functools.lru_cache(maxsize=None)
def bfs_numbered(family, n, seed, nproc, escape=False, done=0.1):
    rng = random.Random(f"bfs-{family}-{n}-{seed}-{nproc}-{escape}-{done}")
    raw = shuffled(FAMILIES[family](n, rng), rng)
    n0 = len(raw)
    escape = escape and nproc > 1 and n0 > 1
    # labels on the raw graph: rows of (process, successor)
    plain = nproc - 1 if escape else nproc
    rows = [[(rng.randrange(plain), j) for j in r] for r in raw]
    if escape:
        for r in rows:
            r.append((nproc - 1, n0))                     # D: one more state, after the raw graph's
        rows.append([(-1, n0)])
    else:
        for v, r in enumerate(rows):
            if not r and rng.random() < done:
                r.append((-1, v))
    # breadth-first from the first `ninit` states, rows in order
    ninit = min(n0, rng.choice((1, 2, 3)))
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
    edges = [[(p, number[j]) for p, j in rows[v]] for v in order]
    m = len(edges)
    en = [{p for p, j in edges[i] if p >= 0 and j != i} for i in range(m)]
    dens = [rng.choice((0.1, 0.5, 0.9)) for _ in PRED_BITS]
    bits = [sum(1 << b for b, d in zip(PRED_BITS, dens) if rng.random() < d) for _ in range(m)]
    if escape:   # D decides most verdicts under a mask with the last process: its own bits are drawn apart from the graph's densities
        bits[number[n0]] = sum(1 << b for b in PRED_BITS if rng.random() < 0.65)
    offsets, dst = csr([[j for _, j in r] for r in edges])
    proc = np.array([p for r in edges for p, _ in r], dtype=np.int8)
    name = f"{family}-{n}-p{nproc}" + ("-escape" if escape else "")
    return Graph(name, m, offsets, dst, proc, np.array(bits, dtype=np.uint32), ninit, level_start, edges, en, bits, nproc)


# ---------------------------------------------------------------------------------------------------------------- the Termination rule
def termination(g, comp, fair_mask):
    """DESIGN section 16 over arrays.  comp[v]: the least state of v's strongly connected component.  Returns (the fair components
    without a Done state as {id: members}, the least id among them or None)"""
    fair = {p for p in range(g.nproc) if fair_mask >> p & 1}
    members = {}
    for v, c in enumerate(comp):
        members.setdefault(c, []).append(v)
    bad = {}
    for c, ms in members.items():
        taken = {p for v in ms for p, j in g.edges[v] if p >= 0 and j != v and comp[j] == c}
        disabled = set().union(*[set(range(g.nproc)) - g.en[v] for v in ms])
        done = any(p < 0 for v in ms for p, _ in g.edges[v])
        if not done and fair <= taken | disabled:
            bad[c] = ms
    return bad, (min(bad) if bad else None)


# ---------------------------------------------------------------------------------------------------------------- the case tables
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
SCC_CASES = [("sparse", n, 1) for n in SIZES + (4099,)] + [("ring_perm", n, 1) for n in SIZES + (4099,)] + \
            [("path", n, 1) for n in (1, 2, 65, 257, 1000)] + [("path_reversed", n, 1) for n in (2, 64, 256, 1000, 4099)] + \
            [("cycle_chain", 268, s) for s in (1, 2, 3)] + [("cycle_chain", 536, 1), ("hub", 1000, 1), ("dense65", 65, 1)] + \
            [("two_level", n, 1) for n in (63, 257, 1000)]

# (family, n, seed, nproc, escape, done)
LIVE_CASES = [
    ("sparse", 1, 1, 1, False, 0.1), ("sparse", 2, 1, 3, False, 1.0), ("sparse", 65, 1, 64, True, 0.1), ("sparse", 257, 2, 3, True, 0.1),
    ("sparse", 1000, 3, 64, True, 0.1), ("sparse", 1000, 4, 1, False, 1.0),
    ("cycle_chain", 268, 1, 1, False, 0.1), ("cycle_chain", 268, 2, 3, True, 0.1), ("cycle_chain", 536, 3, 64, True, 0.1),
    ("two_level", 257, 1, 3, True, 1.0), ("two_level", 1000, 2, 64, True, 0.1), ("two_level", 65, 3, 1, False, 1.0),
    ("ring_perm", 65, 1, 3, True, 0.1), ("ring_perm", 256, 2, 64, True, 0.1), ("ring_perm", 1000, 3, 3, True, 0.1), ("ring_perm", 64, 4, 1, False, 0.1),
]


def case_id(case):
    return "-".join(str(x) for x in case)


def fair_masks(case):
    """0, all, one single bit (the last process: bit 63 of 64) and two random subsets"""
    nproc = case[3]
    rng = random.Random("masks-" + case_id(case))
    full = (1 << nproc) - 1
    return [0, full, 1 << (nproc - 1), rng.getrandbits(nproc), rng.getrandbits(nproc)]


def prop_checks(case):
    """every (kind, p, q, fair mask) asked of the case's graph, in the order asked"""
    return [(kind, p, q, fair) for fair in fair_masks(case) for kind in KINDS for p, q in PQ]


def prop_of(kind, p, q):
    return {"kind": kind, "p": p if kind in (0, 3) else -1, "q": q if kind != 3 else -1}
