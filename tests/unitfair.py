"""Two plain references for liveness under fairness LABEL BY LABEL (`+` / `-` labels), with no engine code
involved.  The rule is restated from the design text, not from liveness.h.  Two notions replace "process":

    unit        the class of an edge: edges[i] = [(unit or -1 for the terminating disjunct, j)]
    conjunct    one WF / SF conjunct of the Spec, a set of units: of_unit[u] = the set of conjuncts unit u belongs to — two for a `+`
                label of a weakly fair process, none for a `-` label or a label of an unfair process

A check is (M, S, T) as in tests/strongfair.py; W / F are the weak / strong CONJUNCTS, disjoint.  For a set X of M that is one state or
strongly connected by its own edges:

    en(s)         the conjuncts k with a step s -> j, j # s, of a unit in k       — in the FULL graph
    taken(X)      the conjuncts k with a step u -> v, u # v, u and v in X, of a unit in k
    disabled(X)   the k with k not in en(s) for some s in X;   enabled(X) the k in en(s) for some s in X
    X is fair     iff  W <= taken(X) | disabled(X)  and  F & enabled(X) <= taken(X)
    violated      iff  some fair X holds a T state and is reachable inside M from an S state of M

decide_units() is the refinement over livegraph.tarjan (components of the open states; closed whole without a T state or with a weak
conjunct neither taken nor disabled; stripped of the states that enable a blocker B = F & enabled \\ taken; else final).
brute_force_units() is the definition over every subset of M.  The two share _conj_stats alone: the three sets of one X."""
import livegraph
import strongfair

TERMINATION = strongfair.TERMINATION
BRUTE_CAP = strongfair.BRUTE_CAP
Units = strongfair.Strong   # violated final ids witness path root rounds closed mask_states bad_starts first_root


def masks_of(of_unit):
    """of_unit as a list of conjunct SETS from a list of masks"""
    return [{k for k in range(64) if m >> k & 1} for m in of_unit]


def en_of(edges, of_unit):
    """en[i]: the conjuncts with a real step in state i"""
    return [set().union(*[of_unit[u] for u, j in row if u >= 0 and j != i]) if row else set() for i, row in enumerate(edges)]


def _conj_stats(X, xs, edges, en, of_unit, nconj):
    taken = set()
    for v in X:
        for u, j in edges[v]:
            if u >= 0 and j != v and j in xs:
                taken |= of_unit[u]
    enabled = set().union(*[en[v] for v in X])
    disabled = set().union(*[set(range(nconj)) - en[v] for v in X])
    return taken, disabled, enabled


def decide_units(edges, of_unit, nconj, ninit, bits, done, prop, weak_mask, strong_mask, rank=None):
    """The refinement.  of_unit: a list of conjunct sets, one per unit.  Returns a Units over state numbers, as
    strongfair.decide_strong returns a Strong."""
    n = len(edges)
    rank = rank or list(range(n))
    M, S, T = strongfair.sets(prop, bits, ninit, done)
    W = {k for k in range(nconj) if weak_mask >> k & 1}
    F = {k for k in range(nconj) if strong_mask >> k & 1}
    assert not W & F
    en = en_of(edges, of_unit)
    OPEN, CLOSED, FINAL = 1, 0, 2
    state = [OPEN if M[v] else CLOSED for v in range(n)]
    final, ids, rounds, closed = [], list(range(n)), 0, 0
    while OPEN in state:
        rounds += 1
        assert rounds <= len(F) + 1, "the refinement did not converge within its bound"
        comp = livegraph.tarjan(n, lambda v: [j for _, j in edges[v] if state[v] == OPEN and state[j] == OPEN])
        groups = {}
        for v in range(n):
            if state[v] == OPEN:
                groups.setdefault(comp[v], []).append(v)
        for ms in groups.values():
            taken, disabled, enabled = _conj_stats(ms, set(ms), edges, en, of_unit, nconj)
            if not any(T[v] for v in ms) or W - taken - disabled:
                for v in ms:
                    state[v] = CLOSED
                closed += len(ms)
                continue
            blockers = (F & enabled) - taken
            if blockers:
                for v in ms:
                    if en[v] & blockers:
                        state[v] = CLOSED
                        closed += 1
                continue
            least = min(ms, key=lambda v: rank[v])
            for v in ms:
                state[v] = FINAL
                ids[v] = least
            final.append(frozenset(ms))
    rounds = max(rounds, 1)
    first_root = min((min(c, key=lambda v: rank[v]) for c in final), key=lambda v: rank[v]) if final else None
    mask_states = sum(M)
    if prop["kind"] == TERMINATION:
        root = next((c for c in final if first_root in c), None)
        return Units(bool(final), set(final), ids, None, [], root, rounds, closed, mask_states, 0, first_root)
    dist = {v: 0 for c in final for v in c}
    level = sorted(dist)
    back = [[] for _ in range(n)]
    for v in range(n):
        for _, j in edges[v]:
            if j != v and M[v] and M[j]:
                back[j].append(v)
    while level:
        nxt = []
        for v in level:
            for u in back[v]:
                if u not in dist:
                    dist[u] = dist[v] + 1
                    nxt.append(u)
        level = nxt
    starts = [v for v in range(n) if S[v] and M[v] and v in dist]
    if not starts:
        return Units(False, set(final), ids, None, [], None, rounds, closed, mask_states, 0, first_root)
    cur = min(starts, key=lambda v: rank[v])
    path = [cur]
    while dist[cur] > 0:
        cur = min((j for _, j in edges[cur] if j != cur and M[j] and dist.get(j) == dist[cur] - 1), key=lambda v: rank[v])
        path.append(cur)
    root = next(c for c in final if cur in c)
    return Units(True, set(final), ids, path[0], path, root, rounds, closed, mask_states, len(starts), first_root)


def brute_force_units(edges, of_unit, nconj, ninit, bits, done, prop, weak_mask, strong_mask):
    """The definition over every non-empty subset of M; None when M holds more than BRUTE_CAP states."""
    n = len(edges)
    M, S, T = strongfair.sets(prop, bits, ninit, done)
    ms = [v for v in range(n) if M[v]]
    if len(ms) > BRUTE_CAP:
        return None
    W = {k for k in range(nconj) if weak_mask >> k & 1}
    F = {k for k in range(nconj) if strong_mask >> k & 1}
    en = en_of(edges, of_unit)
    succ = {v: {j for _, j in edges[v] if j != v and M[j]} for v in ms}
    reach, todo = {v for v in ms if S[v]}, [v for v in ms if S[v]]
    while todo:
        for j in succ[todo.pop()]:
            if j not in reach:
                reach.add(j)
                todo.append(j)

    def spans(X, xs, nbr):
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
        if not xs & reach or not any(T[v] for v in X):
            continue
        if len(X) > 1 and not (spans(X, xs, lambda v: succ[v]) and spans(X, xs, lambda v: [u for u in X if v in succ[u]])):
            continue
        taken, disabled, enabled = _conj_stats(X, xs, edges, en, of_unit, nconj)
        if W <= taken | disabled and F & enabled <= taken:
            return True
    return False


def cycle_meets_every_conjunct(edges, of_unit, nconj, weak_mask, strong_mask, cycle, stutter_state):
    """is the closed walk `cycle` (its last state has an edge back to the first; empty: the behaviour stutters in stutter_state) a fair
    suffix by the definition, and a path of the graph?  Returns None or what is wrong."""
    en = en_of(edges, of_unit)
    X = cycle or [stutter_state]
    steps = list(zip(cycle, cycle[1:] + cycle[:1])) if cycle else []
    taken = set()
    for a, b in steps:
        us = [u for u, j in edges[a] if j == b]
        if not us:
            return f"no edge {a} -> {b}"
        if a != b:
            for u in us:
                if u >= 0:
                    taken |= of_unit[u]
    for k in range(nconj):
        if weak_mask >> k & 1 and k not in taken and all(k in en[v] for v in X):
            return f"weak conjunct {k} is enabled all along and never taken"
        if strong_mask >> k & 1 and k not in taken and any(k in en[v] for v in X):
            return f"strong conjunct {k} is enabled on the walk and never taken"
    return None
