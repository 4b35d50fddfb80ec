"""A plain reference for behaviour checking with unlogged steps (MC_BEH_F_HIDDEN), independent of tla_rust_amd/csrc/behaviour.h.

As tests/behaviours.py, over the same graphs (tests/simgraph.py); the rule is restated from the header of include/tlamc.h:

  * up to H steps that change no observed variable may lie between two observations;
  * C = K_{i-1} closed, depth by depth up to H, under successors that still give observation i - 1 (a flagged successor is no step);
  * every member of C is expanded once: each successor the graph generates counts in `generated`, a flagged one in `errors`; one that
    gives observation i is in K_i (`outside` where it leaves the CONSTRAINT); with `stutter` the members of C that give observation i too;
  * more than 64 states in C at depth d: ambiguous once the members of depth d - 1 are expanded; more than 64 in K_i: ambiguous once
    all of C is; `peak` covers |C| of every observation that is not ambiguous;
  * no hidden step before observation 0.

check() also returns the closures, and path_ok() says whether a path with hidden states is one the graph and the log allow."""
from behaviours import MAX_CANDIDATES, observe
from simgraph import F_ASSERT, F_SPECERR


def check(g, observations, names=None, stutter=False, hidden=0):
    """(verdict dict with mc_beh_verdict's fields, [K_0, K_1, ...], [C_1, C_2, ...] as sets of texts)"""
    v = dict(verdict=None, step=0, candidates=0, peak=0, generated=0, outside=0, errors=0)
    sets, closures, cur = [], [], set()
    for i, o in enumerate(observations):
        nxt = set()
        ambiguous = False
        if i == 0:
            for e in g.init:
                v["generated"] += 1
                if observe(e.text, names) == o:
                    v["outside"] += 0 if e.inmodel else 1
                    nxt.add(e.text)
        else:
            closure, layer, depth = set(cur), set(cur), 0
            while layer:
                new = set()
                for s in layer:
                    if stutter and observe(s, names) == o:
                        nxt.add(s)
                    for e in g.succ[s]:   # (KeyError: a state outside the model; the reference cannot say)
                        v["generated"] += 1
                        if e.flags & (F_ASSERT | F_SPECERR):
                            v["errors"] += 1
                            continue
                        if observe(e.text, names) == o:
                            v["outside"] += 0 if e.inmodel else 1
                            nxt.add(e.text)
                        if depth < hidden and observe(e.text, names) == observations[i - 1] and e.text not in closure:
                            new.add(e.text)
                if len(closure) + len(new) > MAX_CANDIDATES:
                    ambiguous = True
                    break
                closure |= new
                layer, depth = new, depth + 1
            closures.append(closure)
            if not ambiguous and len(nxt) <= MAX_CANDIDATES:
                v["peak"] = max(v["peak"], len(closure))
        if ambiguous or len(nxt) > MAX_CANDIDATES:
            v.update(verdict="ambiguous", step=i)
            return v, sets, closures
        if not nxt:
            v.update(verdict="rejected", step=i)
            return v, sets, closures
        v["candidates"] = len(nxt)
        v["peak"] = max(v["peak"], len(nxt))
        sets.append(nxt)
        cur = nxt
    v.update(verdict="accepted", step=len(observations))
    return v, sets, closures


def compress(texts, names):
    """the log of a walk by an implementation that records only when an observed variable changes: (the states kept, the longest run
    of states dropped between two kept ones)"""
    kept, longest, run = [texts[0]], 0, 0
    for t in texts[1:]:
        if observe(t, names) == observe(kept[-1], names):
            run += 1
        else:
            kept.append(t)
            longest, run = max(longest, run), 0
    return kept, longest   # (a run dropped after the last kept state is no gap: what follows the last observation does not matter)


def path_ok(g, path, observations, names, hidden, stutter=False):
    """path: [(slot, text, obs)].  Every step is an edge of the graph (or, with slot -2, a repeat), every state gives the observation its
    obs names, obs rises by at most one per step from 0, and at most `hidden` states in a row repeat an index"""
    if not path:
        return True
    if path[0][2] != 0 or path[0][0] != -1 or path[0][1] not in g.init_by_text:
        return False
    run = 0
    for k, (slot, text, at) in enumerate(path):
        if observe(text, names) != observations[at]:
            return False
        if k == 0:
            continue
        _, before, was = path[k - 1]
        if slot == -2:
            if not stutter or text != before or at != was + 1:
                return False
        elif text not in {e.text for e in g.succ[before] if not e.flags & (F_ASSERT | F_SPECERR)}:
            return False
        if at == was:
            run += 1
            if run > hidden:
                return False
        elif at == was + 1:
            run = 0
        else:
            return False
    return True
