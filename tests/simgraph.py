"""A plain reference for "is this a legal simulation walk?", independent of tla_rust_amd/csrc/sim_walk.h.

The graph comes from the CPU oracle (oracle/bfs.c, oracle_run_edges: every successor the search generates, with multiplicities) or, for
a compiled PlusCal program, from oracle/tla_eval.py.  The rules are restated from the header of include/tlamc.h ("simulation") and of
sim_walk.h, not from its code:

  * state 1 of a walk is an initial state inside the model (a walk that reached nothing drew an initial state outside it);
  * every step is an edge of the graph to a successor that is inside the CONSTRAINT, differs from its parent and carries no
    Assert / evaluation-error flag;
  * no state of the walk but the last is a violation: it breaks no invariant, none of its successors (in-model or not) fails an
    Assert, raises an evaluation error, breaks a PROPERTY or an invariant, and it has a successor;
  * the walk ends for the reason the graph gives for its last state, in this order: it breaks an invariant itself (violation) —
    it is state number `depth` (depth) — a successor is a violation (violation; of which kind and invariant, and an invariant-breaking
    successor is an edge of the last state) — it has no successor (violation "deadlock" with deadlock checking, else deadlock) — it
    has an in-model, non-stuttering successor (then the walk may not end here) — one successor is a self loop (stutter) — every
    successor is outside the CONSTRAINT (out-of-model);
  * generated = 1 (the initial state) + the successors the graph generates from every state the walk expanded: every state but a
    last one that ended the walk before it was expanded (depth, or an invariant it breaks itself).

`inv_on`: where a lowering checks its INVARIANTs.  "successor": on every enabled successor, in-model or not, when its parent is
expanded (atomic_add, pcal_intro, raft, compiled programs).  "state": once per reached state, when it is expanded, as TLC does per
stored state (paxos, ssi: spec_paxos.h / spec_ssi.h say so in their headers) — there a walk may step into an invariant-breaking state
and must end in it, and successors outside the CONSTRAINT are not checked.  DESIGN.md §13 records this.
"""
import math
from collections import Counter, namedtuple

# the values of include/tlamc.h (MC_SIM_END_*) and of a violation key's kind / slot codes (sim_walk.h's enum, engine_kernels.h VK_*)
END_DEPTH, END_VIOLATION, END_DEADLOCK, END_OUT_OF_MODEL, END_STUTTER = 1, 2, 3, 4, 5
VK_INVARIANT, VK_ASSERT, VK_DEADLOCK, VK_SPECERR = 1, 2, 3, 4
SLOT_NONE, SLOT_INIT, SLOT_PARENT = 0xffff, 0xfffe, 0xfffd
F_ASSERT, F_SPECERR, F_PROPERTY = 1, 2, 4   # oracle/oracle_int.h OR_FLAG_*

Edge = namedtuple("Edge", "text inmodel inv flags action")
INV_ON = {"atomic_add": "successor", "pcal_intro": "successor", "raft": "successor", "pcal": "successor", "paxos": "state", "ssi": "state"}


class WalkError(AssertionError):
    pass


class Graph:
    """init: [Edge] (one per initial state the spec enumerates); succ: {text of an expanded state: [Edge] in generation order}"""

    def __init__(self, init, succ):
        self.init, self.succ = init, succ
        self._passable = {}
        self.init_by_text = {}
        for e in init:
            self.init_by_text.setdefault(e.text, e)
        self.state_inv = {e.text: e.inv for e in init}   # the invariant a state breaks itself (-1: none), from the edges that lead to it
        for es in succ.values():
            for e in es:
                if not e.flags & (F_ASSERT | F_SPECERR):
                    self.state_inv.setdefault(e.text, e.inv)

    def bad_successors(self, s, inv_on):
        """[(kind, invariant index, text)] of the successors of s that are violations"""
        out = []
        for e in self.succ[s]:
            if e.flags & F_ASSERT:
                out.append((VK_ASSERT, 0, None))
            elif e.flags & F_SPECERR:
                out.append((VK_SPECERR, 0, None))
            elif e.flags & F_PROPERTY:
                out.append((VK_INVARIANT, e.flags >> 8, e.text))
            elif e.inv >= 0 and inv_on == "successor":
                out.append((VK_INVARIANT, e.inv, e.text))
        return out

    def passable(self, s, inv_on):
        """(successors generated, texts a walk may step to) of a state a walk may pass through, else None; kept per state"""
        key = (s, inv_on)
        if key not in self._passable:
            ok = s in self.succ and self.state_inv[s] < 0 and self.succ[s] and not self.bad_successors(s, inv_on)
            steps = Counter(e.text for e in self.succ[s] if not e.flags & (F_ASSERT | F_SPECERR)) if ok else None
            outside = {e.text for e in self.succ[s] if not e.inmodel} if ok else None
            self._passable[key] = (len(self.succ[s]), frozenset(t for t in steps if t != s and t not in outside)) if ok else None
        return self._passable[key]

    def candidates(self, s):
        """{successor text: multiplicity} over the in-model, non-stuttering, unflagged successors of s"""
        return Counter(e.text for e in self.succ[s] if not e.flags & (F_ASSERT | F_SPECERR) and e.inmodel and e.text != s)


def from_oracle_files(dump_path, edges_path):
    """Graph from the oracle's state dump ("L<level> <text>", line k = state k) and edge dump (oracle/oracle.h oracle_run_edges)"""
    with open(dump_path) as f:
        states = [line.rstrip("\n").split(" ", 1)[1] for line in f]
    init, succ = [], {t: [] for t in states}
    with open(edges_path) as f:
        for line in f:
            par, action, flags, inmodel, inv, text = line.rstrip("\n").split(" ", 5)
            e = Edge(text, int(inmodel) == 1, int(inv), int(flags), int(action))
            (init if par == "-1" else succ[states[int(par)]]).append(e)
    return Graph(init, succ)


def from_checker(ck, invariants=(), constraints=()):
    """Graph of a module under oracle/tla_eval.py's Checker: every state reachable through in-model states"""
    ck.engine_mode = True

    def edge(s, action=0):
        if "__assert__" in s:
            return Edge("-", False, -1, F_ASSERT, action), None
        inv = next((k for k, name in enumerate(invariants) if not ck.ev(ck.defs[name][1], s, None, {})), -1)
        return Edge(ck.fmt_state(s).replace("\n", " "), bool(ck.in_model(s, constraints)), inv, 0, action), s
    init, succ, todo = [], {}, []
    for s in ck.initial_states():
        e, st = edge(s, -1)
        init.append(e)
        todo.append((e, st))
    while todo:
        e, st = todo.pop()
        if st is None or not e.inmodel or e.text in succ:
            continue
        out = succ[e.text] = []
        for n in ck.successors(st):
            e2, st2 = edge(n)
            out.append(e2)
            todo.append((e2, st2))
    ck.engine_mode = False
    return Graph(init, succ)


def check_walk(g, texts, end, depth, deadlock, inv_on, viol=None, viol_succ=None):
    """texts: the one-line texts of the states the walk reached; end: MC_SIM_END_*; viol: (kind, invariant, slot code) of its violation
    key or None; viol_succ: text of the successor that broke an invariant.  Returns the `generated` the graph gives the walk; raises
    WalkError when the walk is not one the graph allows."""
    def fail(msg):
        raise WalkError(f"{msg} [len {len(texts)}, end {end}, depth {depth}, deadlock {deadlock}, viol {viol}]")

    def need_viol(kinds):
        if end != END_VIOLATION:
            fail(f"the graph ends this walk on a violation {kinds}")
        if viol is None:
            fail("a walk that ended on a violation has no violation key")
        if (viol[0], viol[1]) not in {(k, i) for k, i, _ in kinds}:
            fail(f"violation {viol[:2]} is not one the graph gives the last state: {[(k, i) for k, i, _ in kinds]}")
    n = len(texts)
    if end != END_VIOLATION and viol is not None:
        fail("a violation key on a walk that ended otherwise")
    if n == 0:
        if end != END_OUT_OF_MODEL or not any(not e.inmodel for e in g.init):
            fail("only a walk whose initial state is outside the model reaches nothing")
        return 1
    if n > depth:
        fail("more states than depth")
    e0 = g.init_by_text.get(texts[0])
    if e0 is None:
        fail(f"state 1 is not an initial state: {texts[0]}")
    if e0.inv < 0 and not e0.inmodel:
        fail("state 1 is outside the model")
    gen = 1
    for k in range(n - 1):
        s = texts[k]
        fast = g.passable(s, inv_on)   # (the checks below, made once per state: None when one of them fails, then they say which)
        if fast is not None and texts[k + 1] in fast[1]:
            gen += fast[0]
            continue
        if s not in g.succ:
            fail(f"state {k + 1} is not a state of the graph: {s}")
        if g.state_inv[s] >= 0:
            fail(f"state {k + 1} breaks invariant {g.state_inv[s]} and the walk went on")
        bad = g.bad_successors(s, inv_on)
        if bad:
            fail(f"state {k + 1} has a violating successor {bad[0][:2]} and the walk went on")
        if not g.succ[s]:
            fail(f"state {k + 1} has no successor and the walk went on")
        if texts[k + 1] == s:
            fail(f"step {k + 1} stutters")
        step = [e for e in g.succ[s] if e.text == texts[k + 1] and not e.flags & (F_ASSERT | F_SPECERR)]
        if not step:
            fail(f"step {k + 1} is not an edge of the graph: {s} -> {texts[k + 1]}")
        if not all(e.inmodel for e in step):
            fail(f"step {k + 1} leaves the model")
        gen += len(g.succ[s])
    s = texts[-1]
    if s not in g.state_inv:
        fail(f"the last state is not a state of the graph: {s}")
    if g.state_inv[s] >= 0 and (inv_on == "state" or n == 1):
        need_viol([(VK_INVARIANT, g.state_inv[s], None)])
        if viol[2] != (SLOT_INIT if n == 1 and inv_on == "successor" else SLOT_PARENT):
            fail("an invariant the last state breaks itself is reported with another slot code")
        return gen
    if g.state_inv[s] >= 0:
        fail(f"the last state breaks invariant {g.state_inv[s]}: its parent had to end the walk")
    if s not in g.succ:
        fail(f"the last state is not a state the search stores: {s}")
    if n == depth:
        if end != END_DEPTH:
            fail("the walk has depth states and another end reason")
        return gen
    if end == END_DEPTH:
        fail("end reason depth on a walk of fewer states")
    gen += len(g.succ[s])
    bad = g.bad_successors(s, inv_on)
    if bad:
        need_viol(bad)
        if viol[0] == VK_INVARIANT:
            if viol[2] >= SLOT_PARENT:
                fail("an invariant broken by a successor is reported without its slot")
            if viol_succ is not None and (VK_INVARIANT, viol[1], viol_succ) not in bad:
                fail(f"the invariant-breaking successor is not an edge of the last state: {viol_succ}")
        return gen
    if not g.succ[s]:
        if deadlock:
            need_viol([(VK_DEADLOCK, 0, None)])
            if viol[2] != SLOT_NONE:
                fail("a deadlock is reported with a slot")
        elif end != END_DEADLOCK:
            fail("the last state has no successor, deadlock checking is off, and the end reason is not deadlock")
        return gen
    if g.candidates(s):
        fail("the walk ended at a state that has an in-model, non-stuttering successor")
    want = END_STUTTER if any(e.text == s for e in g.succ[s]) else END_OUT_OF_MODEL
    if end != want:
        fail(f"the graph gives end reason {want}")
    return gen


def key_fields(key):
    """(kind, invariant index, slot code) of a violation key (sim_walk.h sim_key: walk << 24 | slot << 8 | inv << 3 | kind), None for None"""
    return None if key is None else (key & 7, (key >> 3) & 31, (key >> 8) & 0xffff)


def check_run(g, run, texts, depth, deadlock, inv_on, totals=True):
    """every walk of a host run (simwalk.walks(..., dump=...), texts = simwalk.walk_texts) against the graph, and the run's counters
    against the sums over its walks.  Returns Counter of end reasons."""
    ends, gen, memo = Counter(), 0, {}
    for w, (tx, succ) in zip(run["walks"], texts):
        key = (tuple(tx), w["end"], key_fields(w["viol"]), succ)   # (equal walks are judged once: a million short walks are few distinct ones)
        want = memo.get(key)
        if want is None:
            want = memo[key] = check_walk(g, tx, w["end"], depth, deadlock, inv_on, viol=key[2], viol_succ=succ)
        if "gen" in w and w["gen"] != want:
            raise WalkError(f"the walk's generated is {w['gen']}, the graph gives {want} [len {w['len']}, end {w['end']}]")
        gen += want
        ends[w["end"]] += 1
    if totals:
        got = (run["generated"], run["steps"], run["walks_done"], run["max_depth"])
        want = (gen, sum(len(tx) for tx, _ in texts), len(texts), max((len(tx) for tx, _ in texts), default=0))
        if got != want:
            raise WalkError(f"run totals (generated, steps, walks, max_depth) {got}, the graph gives {want}")
        keys = [w["viol"] for w in run["walks"] if w["viol"] is not None]
        if run["viol"] != (min(keys) if keys else None):
            raise WalkError("the run's violation is not the least key of its walks")
    return ends


# ------------------------------------------------------------------------------------------------ chi-square, without scipy
def gammaq(a, x):
    """regularised upper incomplete gamma function Q(a, x) (series for x < a + 1, continued fraction otherwise)"""
    if x <= 0:
        return 1.0
    if x < a + 1:
        term = total = 1.0 / a
        k = a
        while abs(term) > abs(total) * 1e-16:
            k += 1
            term *= x / k
            total += term
        return 1.0 - total * math.exp(-x + a * math.log(x) - math.lgamma(a))
    tiny = 1e-300
    b = x + 1 - a
    c = 1 / tiny
    d = 1 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1 / d
        delta = d * c
        h *= delta
        if abs(delta - 1) < 1e-16:
            break
    return math.exp(-x + a * math.log(x) - math.lgamma(a)) * h


def chi2_sf(x, df):
    return gammaq(df / 2.0, x / 2.0)


def chi2_critical(df, alpha):
    """x with P(chi-square_df > x) = alpha, by bisection on chi2_sf"""
    lo, hi = 0.0, float(df)
    while chi2_sf(hi, df) > alpha:
        hi *= 2
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if chi2_sf(mid, df) > alpha else (lo, mid)
    return hi


def chi2_stat(observed, weights):
    """(statistic, degrees of freedom) of observed counts {cell: n} against probabilities proportional to weights {cell: w}; every
    expected count must be at least 5 and nothing may be observed outside the weighted cells"""
    total, wsum = sum(observed.values()), sum(weights.values())
    assert set(observed) <= set(weights), set(observed) - set(weights)
    stat = 0.0
    for cell, w in weights.items():
        exp = total * w / wsum
        assert exp >= 5, (cell, exp)
        stat += (observed.get(cell, 0) - exp) ** 2 / exp
    return stat, len(weights) - 1
