"""A plain reference for <>Q, []<>Q, <>[]P and P ~> Q under weak process fairness, with no engine code involved.  It builds on
tests/livegraph.py's LiveGraph (the state graph of a PlusCal module under oracle/tla_eval.py, with the process of every edge) and
evaluates the predicates of the program's properties with the same evaluator: one definition LivePred_k per predicate is appended to the
translation, as LiveP_k is.  The rule is restated from DESIGN.md section 17, not from liveness.h.  A check is a triple of state sets:

    kind                     M                S                        T
    0  P ~> Q                ~Q               P /\\ ~Q                  all
    1  []<>Q                 ~Q               ~Q                       all
    2  <>Q                   ~Q               initial states with ~Q   all
    3  <>[]P                 all              all                      ~P

    G[M]          the subgraph induced by M; C ranges over its strongly connected components, one-state components included
    taken(C)      the p with a step u -> v, u # v, u and v in C
    disabled(C)   the p with ~en(s, p) for some s in C — en in the FULL graph: a step that leaves M still enables its process
    violated      iff some C is fair (every fair p in taken(C) or disabled(C)), holds a T state and is reachable inside M from an S
                  state that is itself in M

What this reference does NOT check: it takes each check's kind, P and Q — and each predicate's text — from the front end under test
(Program.live_properties / live_predicates), so a definition classified as another formula than the one written is invisible to it and
to every test built on it.  Classification is guarded by the hand-written tables of tests/test_liveprops_host.py alone (ACCEPTED,
REFUSED: operator precedence around the temporal operators included).

decide() is that rule with livegraph.tarjan on the induced subgraph; brute_force() is the definition without the component shortcut:
every non-empty subset of M that is one state or strongly connected by its own edges.  The least-index rules of the engine (witness,
the way from it into a component) take the order of the system under test as `rank`."""
import sys
from collections import namedtuple

import helpers
import livegraph

sys.path.insert(0, str(helpers.ROOT / "oracle"))

DIR = helpers.ROOT / "specs_liveprops"
LEADS_TO, INF_OFTEN, EVENTUALLY, STABLE = range(4)

# name -> (module file, cfg file, constants, the process instances' actions in slot order, {check name: is it violated?})  — the last
# column is what the model was WRITTEN to show (its file's comment argues it); test_liveprops_host.py checks the reference against it
# before anything relies on the reference
Model = namedtuple("Model", "tla cfg constants procs expect")
MODELS = {
    # 1 leaving counts as enabled
    "leave_enabled": Model("leave_enabled.tla", "leave_enabled.cfg", {}, ["Spin", "Leave"], {"Reaches": False}),
    "leave_enabled_unfair": Model("leave_enabled_unfair.tla", "leave_enabled_unfair.cfg", {}, ["Spin", "Leave"], {"Reaches": True}),
    # 2 the mask splits a component
    "mask_split": Model("mask_split.tla", "mask_split.cfg", {}, ["Ring"], {"Recurs": False}),
    # 3 reach respects the mask
    "reach_mask": Model("reach_mask.tla", "reach_mask.cfg", {}, ["Walk"], {"Through": False, "Inside": True}),
    # 4 <>[]P
    "stable": Model("stable.tla", "stable.cfg", {}, ["Flip"], {"Settles": True}),
    "stable_transient": Model("stable_transient.tla", "stable_transient.cfg", {}, ["Up"], {"Settles": False}),
    # 5 <>Q versus []<>Q
    "lost": Model("lost.tla", "lost.cfg", {}, ["Lose"], {"Once": False, "Again": True}),
    # 6 a stuttering witness
    "stutter": Model("stutter.tla", "stutter.cfg", {}, ["Step"], {"Never": True}),
    # 7 starvation under WF; two instances from one definition
    "starve_leads": Model("starve_leads.tla", "starve_leads.cfg", {}, ["Waiter", "Flipper"], {"Served": True}),
    "peterson_loop": Model("peterson_loop.tla", "peterson_loop.cfg", {}, ["Proc(0)", "Proc(1)"], {"Starvation[i = 0]": False, "Starvation[i = 1]": False}),
    # 8 sizes (the 1000-ring is for the GPU alone: tests/test_gpu_liveprops.py takes Tarjan to the engine's own arrays)
    "ring_cut": Model("ring_cut.tla", "ring_cut.cfg", {"N": 65, "Half": 32}, ["Counter", "Stopper"], {"Cut": True}),
}
SMALL = [n for n in MODELS if n != "ring_cut"]   # models 1 - 7: every check's M holds at most BRUTE_CAP states
BRUTE_CAP = 14
# 9 refusals: file -> (property, the reason's key word)
REFUSED = {"refused_nested": ("Deep", "nested"), "refused_exists": ("Some", "\\E"), "refused_subset": ("Odd", "subset"), "refused_many": ("Many", "16 checks")}


def compiled(stem, cfg=None):
    import tla_rust_amd as amd
    return amd.Program((DIR / (stem + ".tla")).read_text(), (DIR / ((cfg or stem) + ".cfg")).read_text())


def predicate_text(key):
    """a predicate of Program.live_predicates — its tokens joined by blanks, then ` | x = v` per quantifier variable it mentions — as
    a TLA+ expression: the variables replaced by their values, token by token"""
    text, *bound = key.split(" | ")
    vals = dict(b.split(" = ", 1) for b in bound)
    return " ".join(vals.get(t, t) for t in text.split(" "))


class PropGraph(livegraph.LiveGraph):
    """LiveGraph plus bits[i]: bit k = predicate k of the program holds in state i, evaluated by oracle/tla_eval.py on the states
    found by a walk of its own (matched to the LiveGraph's by their text)"""

    def __init__(self, program, model):
        super().__init__(program, model)
        from tla_eval import Checker
        text = program.translated()
        preds = list(program.live_predicates)
        extra = "".join(f"LivePred_{k} == {predicate_text(p)}\n" for k, p in enumerate(preds))
        at = text.rindex("\n====") + 1
        ck = Checker(text[:at] + extra + text[at:], constants=dict(model.constants))

        def line(s):
            return ck.fmt_state(s).replace("\n", " ")
        self.bits = [None] * len(self.texts)
        todo = list(ck.initial_states())
        while todo:
            s = todo.pop()
            i = self.index[line(s)]
            if self.bits[i] is not None:
                continue
            self.bits[i] = sum(1 << k for k in range(len(preds)) if ck.ev(ck.defs[f"LivePred_{k}"][1], s, None, {}))
            todo.extend(ck.successors(s))
        assert all(b is not None for b in self.bits)


def load(name):
    """(Program, PropGraph) of a model of MODELS; the caller closes the program"""
    m = MODELS[name]
    prog = compiled(m.tla[:-4], m.cfg[:-4])
    return prog, PropGraph(prog, m)


def sets(kind, p, q, bits, ninit):
    """(M, S, T) as lists of booleans, one per state; the initial states are 0 .. ninit - 1"""
    n = len(bits)

    def has(k, i):
        return bool(bits[i] >> k & 1)
    if kind == STABLE:
        return [True] * n, [True] * n, [not has(p, i) for i in range(n)]
    M = [not has(q, i) for i in range(n)]
    if kind == LEADS_TO:
        S = [M[i] and has(p, i) for i in range(n)]
    elif kind == INF_OFTEN:
        S = list(M)
    else:
        S = [M[i] and i < ninit for i in range(n)]
    return M, S, [True] * n


Verdict = namedtuple("Verdict", "violated violating witness path root mask_states bad_starts comp")


def decide(edges, en, nproc, ninit, bits, prop, fair_mask, rank=None):
    """The rule.  edges[i] = [(process or -1, j)], en[i] = the processes with a real step in state i (full graph).  rank[i]: the
    index the system under test gives state i (default: i).  Returns a Verdict over state NUMBERS: violating = the violating
    components as frozensets; witness = the S state of least rank from which one is reached inside M; path = from the witness along
    strictly falling distance, the successor of least rank each time; root = the component the path ends in; comp[i] = the least
    member (by number) of state i's component of G[M], a state outside M being a component of its own."""
    n = len(edges)
    rank = rank or list(range(n))
    M, S, T = sets(prop["kind"], prop["p"], prop["q"], bits, ninit)
    fair = {k for k in range(nproc) if fair_mask >> k & 1}
    comp = livegraph.tarjan(n, lambda v: [j for _, j in edges[v] if M[v] and M[j]])
    members = {}
    for v in range(n):
        if M[v]:
            members.setdefault(comp[v], []).append(v)
    violating = []
    for c, ms in members.items():
        taken = {k for v in ms for k, j in edges[v] if k >= 0 and j != v and M[j] and comp[j] == c}
        disabled = set().union(*[set(range(nproc)) - en[v] for v in ms])
        if fair <= taken | disabled and any(T[v] for v in ms):
            violating.append(frozenset(ms))
    # distance to a violating component inside M: breadth-first over the reversed edges
    dist = [None] * n
    level = sorted(v for c in violating for v in c)
    for v in level:
        dist[v] = 0
    pred = [[] for _ in range(n)]
    for v in range(n):
        for _, j in edges[v]:
            if j != v and M[v] and M[j]:
                pred[j].append(v)
    d = 0
    while level:
        d += 1
        nxt = []
        for v in level:
            for u in pred[v]:
                if dist[u] is None:
                    dist[u] = d
                    nxt.append(u)
        level = nxt
    starts = [v for v in range(n) if S[v] and M[v] and dist[v] is not None]
    if not starts:
        return Verdict(False, set(violating), None, [], None, sum(M), 0, comp)
    cur = min(starts, key=lambda v: rank[v])
    path = [cur]
    while dist[cur] > 0:
        cur = min((j for _, j in edges[cur] if j != cur and M[j] and dist[j] == dist[cur] - 1), key=lambda v: rank[v])
        path.append(cur)
    root = next(c for c in violating if cur in c)
    return Verdict(True, set(violating), path[0], path, root, sum(M), len(starts), comp)


def decide_model(g, prop, fair_mask, rank=None):
    return decide(g.edges, g.en, g.nproc, len(g.init), g.bits, prop, fair_mask, rank)


def brute_force(g, prop, fair_mask):
    """The definition, sharing nothing with the component shortcut: is there a non-empty subset X of M that is a single state or
    strongly connected by its own edges, fair by its own taken / disabled sets, holds a T state and is reachable inside M from an S
    state of M?  None when M holds more than BRUTE_CAP states."""
    n = len(g.edges)
    M, S, T = sets(prop["kind"], prop["p"], prop["q"], g.bits, len(g.init))
    ms = [v for v in range(n) if M[v]]
    if len(ms) > BRUTE_CAP:
        return None
    fair = {k for k in range(g.nproc) if fair_mask >> k & 1}
    succ = {v: {j for _, j in g.edges[v] if j != v and M[j]} for v in ms}
    reach = set(v for v in ms if S[v])   # the states reachable inside M from an S state of M
    todo = list(reach)
    while todo:
        for j in succ[todo.pop()]:
            if j not in reach:
                reach.add(j)
                todo.append(j)

    def connected(X, nbr):
        seen, todo = {X[0]}, [X[0]]
        while todo:
            for j in nbr(todo.pop()):
                if j in xs and j not in seen:
                    seen.add(j)
                    todo.append(j)
        return len(seen) == len(X)
    for code in range(1, 1 << len(ms)):
        X = [ms[k] for k in range(len(ms)) if code >> k & 1]
        xs = set(X)
        if not (xs & reach) or not any(T[v] for v in X):
            continue
        if len(X) > 1 and not (connected(X, lambda v: succ[v]) and connected(X, lambda v: [u for u in X if v in succ[u]])):
            continue
        taken = {k for v in X for k, j in g.edges[v] if k >= 0 and j != v and j in xs}
        disabled = set().union(*[set(range(g.nproc)) - g.en[v] for v in X])
        if fair <= taken | disabled:
            return True
    return False
