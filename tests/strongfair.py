"""Two plain references for liveness under weak AND strong process fairness (`fair+ process`), with no engine code involved.  The rule
is restated from DESIGN.md section 19, not from liveness.h.  A check is (M, S, T) as in tests/liveprops.py (`Termination`: M = all, S =
the initial states, T = the states that are not Done); Fair is split into W (weak) and F (strong), disjoint.  For a set X of M that is
one state or strongly connected by its own edges:

    taken(X)      the p with a step u -> v, u # v, u and v in X
    disabled(X)   the p with ~en(s, p) for some s in X      — en in the FULL graph
    enabled(X)    the p with  en(s, p) for some s in X
    X is fair     iff  W <= taken(X) | disabled(X)  and  F & enabled(X) <= taken(X)
    violated      iff  some fair X holds a T state and is reachable inside M from an S state of M

decide_strong() is the refinement over livegraph.tarjan: components of the open states; a component without a T state or with a weak
process neither taken nor disabled somewhere is closed whole; one with blockers B = F & enabled \\ taken loses the states that enable a
process of B; any other is final.  brute_force_strong() is the definition over every subset of M, sharing nothing with the refinement.
`Termination` is decided as DESIGN section 16 decides it, without a reach pass: every state of a state graph is reachable from an
initial state (the brute force does walk from S; the two agree on graphs of reachable states).  The least-index rules of the engine (witness, the way from it into a component, the least final root) take the order of the system
under test as `rank`."""
from collections import namedtuple

import livegraph
import liveprops

DIR = liveprops.helpers.ROOT / "specs_strongfair"
TERMINATION = -1
BRUTE_CAP = liveprops.BRUTE_CAP

# name -> (module file, cfg file, constants, the process instances' actions in slot order, {check name: is it violated under the model's
# own fairness keywords?})  — the last column is what the model was WRITTEN to show (its file's comment argues it)
Model = liveprops.Model
MODELS = {
    "sem2_fair": Model("sem2_fair.tla", "sem2_fair.cfg", {}, ["P(0)", "P(1)"], {"Served[i = 0]": True, "Served[i = 1]": True}),
    "sem2_strong": Model("sem2_strong.tla", "sem2_strong.cfg", {}, ["P(0)", "P(1)"], {"Served[i = 0]": False, "Served[i = 1]": False}),
    "sem3_fair": Model("sem3_fair.tla", "sem3_fair.cfg", {}, ["P(0)", "P(1)", "P(2)"], {f"Served[i = {i}]": True for i in range(3)}),
    "sem3_strong": Model("sem3_strong.tla", "sem3_strong.cfg", {}, ["P(0)", "P(1)", "P(2)"], {f"Served[i = {i}]": False for i in range(3)}),
    "toggle_fair": Model("toggle_fair.tla", "toggle_fair.cfg", {}, ["Waiter", "Toggler"], {"Termination": True}),
    "toggle_strong": Model("toggle_strong.tla", "toggle_strong.cfg", {}, ["Waiter", "Toggler"], {"Termination": False}),
    "subcycle": Model("subcycle.tla", "subcycle.cfg", {}, ["Exit", "Walk"], {"Termination": True, "Leaves": True, "Gone": True}),
    "mixed_sf": Model("mixed_sf.tla", "mixed_sf.cfg", {}, ["Waiter", "Flipper", "Noise"], {"Gets": False}),
    "mixed_wf": Model("mixed_wf.tla", "mixed_wf.cfg", {}, ["Waiter", "Flipper", "Noise"], {"Gets": True}),
    "mixed_noise": Model("mixed_noise.tla", "mixed_noise.cfg", {}, ["Waiter", "Flipper", "Noise"], {"Gets": True}),
    "leftover": Model("leftover.tla", "leftover.cfg", {}, ["Kick", "Flip"], {"Settles": True, "Kicked": True}),
    "ring_strong": Model("ring_strong.tla", "ring_strong.cfg", {"N": 65, "Half": 32}, ["Counter", "Stopper"], {"Termination": False, "Stops": False}),
}
# (the 1000-ring is for the GPU alone: tests/test_gpu_strongfair.py takes the reference to the engine's own arrays)
SMALL = [n for n in MODELS if n != "ring_strong"]
ROUNDS = {"subcycle": 2, "leftover": 2, "ring_strong": 2, "toggle_strong": 2}   # the rounds every check of the model takes
REFUSED = {"refused_strong_label": "modifier"}   # still refused under the strong entry


def compiled(stem, cfg=None):
    import tla_rust_amd as amd
    return amd.Program((DIR / (stem + ".tla")).read_text(), (DIR / ((cfg or stem) + ".cfg")).read_text())


class StrongGraph(liveprops.PropGraph):
    """PropGraph of a model of specs_strongfair (the predicates' bits are empty for a cfg with Termination alone)"""


def load(name):
    """(Program, StrongGraph, the checks of its cfg) of a model of MODELS; the caller closes the program"""
    m = MODELS[name]
    prog = compiled(m.tla[:-4], m.cfg[:-4])
    return prog, StrongGraph(prog, m), checks_of(prog, (DIR / m.cfg).read_text())


def checks_of(prog, cfg_text):
    """every check of a program's cfg as (name, prop): prop is a dict with kind / p / q, kind TERMINATION for `Termination`"""
    out = [(lp["name"], lp) for lp in prog.live_properties if not lp["refused"]]
    if "PROPERTY Termination" in cfg_text:
        out.insert(0, ("Termination", {"kind": TERMINATION, "p": -1, "q": -1}))
    return out


def sets(prop, bits, ninit, done):
    """(M, S, T), one boolean per state"""
    n = len(done)
    if prop["kind"] == TERMINATION:
        return [True] * n, [i < ninit for i in range(n)], [not d for d in done]
    return liveprops.sets(prop["kind"], prop["p"], prop["q"], bits, ninit)


def _bitset(mask, nproc):
    return {k for k in range(nproc) if mask >> k & 1}


def _stats(X, xs, edges, en, nproc):
    taken = {k for v in X for k, j in edges[v] if k >= 0 and j != v and j in xs}
    enabled = set().union(*[en[v] for v in X])
    disabled = set().union(*[set(range(nproc)) - en[v] for v in X])
    return taken, disabled, enabled


Strong = namedtuple("Strong", "violated final ids witness path root rounds closed mask_states bad_starts first_root")


def decide_strong(edges, en, nproc, ninit, bits, done, prop, weak_mask, strong_mask, rank=None):
    """The refinement.  edges[i] = [(process or -1, j)], en[i] = the processes with a real step in state i (full graph), done[i].
    Returns a Strong over state NUMBERS: final = the final violating components as frozensets; ids[i] = the refined id (the least
    member — by rank — of i's final component, i itself for every other state); witness / path / root as liveprops.decide (for
    Termination: no witness, root = the final component of least id); rounds; closed = the number of states of M closed."""
    n = len(edges)
    rank = rank or list(range(n))
    M, S, T = sets(prop, bits, ninit, done)
    W, F = _bitset(weak_mask, nproc), _bitset(strong_mask, nproc)
    assert not W & F
    state = [1 if M[v] else 0 for v in range(n)]   # 1 open, 0 closed, 2 final
    final, ids, rounds, closed = [], list(range(n)), 0, 0
    while any(s == 1 for s in state):
        rounds += 1
        assert rounds <= len(F) + 1, "the refinement did not converge within its bound"
        comp = livegraph.tarjan(n, lambda v: [j for _, j in edges[v] if state[v] == 1 and state[j] == 1])
        members = {}
        for v in range(n):
            if state[v] == 1:
                members.setdefault(comp[v], []).append(v)
        for ms in members.values():
            xs = set(ms)
            taken, disabled, enabled = _stats(ms, xs, edges, en, nproc)
            if not any(T[v] for v in ms) or not W <= taken | disabled:
                for v in ms:
                    state[v] = 0
                closed += len(ms)
                continue
            B = (F & enabled) - taken
            if B:
                for v in ms:
                    if en[v] & B:
                        state[v] = 0
                        closed += 1
                continue
            least = min(ms, key=lambda v: rank[v])
            for v in ms:
                state[v] = 2
                ids[v] = least
            final.append(frozenset(ms))
    rounds = max(rounds, 1)
    first_root = min((min(c, key=lambda v: rank[v]) for c in final), key=lambda v: rank[v]) if final else None
    mask_states = sum(M)
    if prop["kind"] == TERMINATION:
        root = next((c for c in final if first_root in c), None)
        return Strong(bool(final), set(final), ids, None, [], root, rounds, closed, mask_states, 0, first_root)
    # distance to a final component inside M: breadth-first over the reversed edges
    dist = [None] * n
    level = sorted(v for c in final for v in c)
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
        return Strong(False, set(final), ids, None, [], None, rounds, closed, mask_states, 0, first_root)
    cur = min(starts, key=lambda v: rank[v])
    path = [cur]
    while dist[cur] > 0:
        cur = min((j for _, j in edges[cur] if j != cur and M[j] and dist[j] == dist[cur] - 1), key=lambda v: rank[v])
        path.append(cur)
    root = next(c for c in final if cur in c)
    return Strong(True, set(final), ids, path[0], path, root, rounds, closed, mask_states, len(starts), first_root)


def decide_model(g, prop, weak_mask, strong_mask, rank=None):
    return decide_strong(g.edges, g.en, g.nproc, len(g.init), g.bits, g.done, prop, weak_mask, strong_mask, rank)


def brute_force_strong(edges, en, nproc, ninit, bits, done, prop, weak_mask, strong_mask):
    """The definition: is there a non-empty subset X of M, one state or strongly connected by its own edges, fair by its own taken /
    disabled / enabled sets, with a T state, reachable inside M from an S state of M?  None when M holds more than BRUTE_CAP states."""
    n = len(edges)
    M, S, T = sets(prop, bits, ninit, done)
    ms = [v for v in range(n) if M[v]]
    if len(ms) > BRUTE_CAP:
        return None
    W, F = _bitset(weak_mask, nproc), _bitset(strong_mask, nproc)
    succ = {v: {j for _, j in edges[v] if j != v and M[j]} for v in ms}
    reach = set(v for v in ms if S[v])
    todo = list(reach)
    while todo:
        for j in succ[todo.pop()]:
            if j not in reach:
                reach.add(j)
                todo.append(j)

    def connected(X, xs, nbr):
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
        if len(X) > 1 and not (connected(X, xs, lambda v: succ[v]) and connected(X, xs, lambda v: [u for u in X if v in succ[u]])):
            continue
        taken, disabled, enabled = _stats(X, xs, edges, en, nproc)
        if W <= taken | disabled and F & enabled <= taken:
            return True
    return False

