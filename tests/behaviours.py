"""A plain reference for "is this recorded behaviour a behaviour of the model?", independent of tla_rust_amd/csrc/behaviour.h.

The graph is tests/simgraph.py's (the CPU oracle's edge-labelled state graph, or oracle/tla_eval.py's for a compiled program); the rule
is restated from the header of include/tlamc.h ("recorded behaviours"), not from the code:

  * an observation says what some variables are (all of them: the state's text); a state matches it when it agrees on those;
  * K_0 = the initial states that match observation 0; K_i = the states that match observation i and are a successor of a member of
    K_{i-1} — with `stutter` also the members of K_{i-1} that match;
  * a successor flagged Assert / evaluation error is no step (errors); one outside the CONSTRAINT is (outside, where it matches);
    invariants do not matter;
  * accepted when the last set is non-empty, rejected at the first empty set, ambiguous at the first set of more than 64 states;
  * generated = the initial states + every successor the graph generates from a member of a set that was expanded.

Candidate sets are sets of graph nodes (state texts); masks are given by variable name."""
import re

from simgraph import F_ASSERT, F_SPECERR

MAX_CANDIDATES = 64


def variables_of(text):
    """{variable: value text} of a state text "/\\ a = 1 /\\ b = <<2, 3>>" (one line)"""
    out = {}
    for part in re.split(r"(?:^|\s)/\\\s", text):
        if part.strip():
            name, _, value = part.partition(" = ")
            out[name.strip()] = value.strip()
    return out


def observe(text, names=None):
    """what a log of the variables `names` (None: all) records of the state"""
    if names is None:
        return text
    v = variables_of(text)
    return tuple((n, v[n]) for n in sorted(names))


def check(g, observations, names=None, stutter=False):
    """(verdict dict with mc_beh_verdict's fields, [K_0, K_1, ...] as sets of texts) for observations made with observe(., names)"""
    v = dict(verdict=None, step=0, candidates=0, peak=0, generated=0, outside=0, errors=0)
    sets, cur = [], set()
    for i, o in enumerate(observations):
        nxt = set()
        if i == 0:
            for e in g.init:
                v["generated"] += 1
                if observe(e.text, names) == o:
                    v["outside"] += 0 if e.inmodel else 1
                    nxt.add(e.text)
        else:
            for s in cur:
                if stutter and observe(s, names) == o:
                    nxt.add(s)
                for e in g.succ[s]:   # (KeyError: the graph never expanded s — a state outside the model; the reference cannot say)
                    v["generated"] += 1
                    if e.flags & (F_ASSERT | F_SPECERR):
                        v["errors"] += 1
                    elif observe(e.text, names) == o:
                        v["outside"] += 0 if e.inmodel else 1
                        nxt.add(e.text)
        if len(nxt) > MAX_CANDIDATES:
            v.update(verdict="ambiguous", step=i)
            return v, sets
        if not nxt:
            v.update(verdict="rejected", step=i)
            return v, sets
        v["candidates"] = len(nxt)
        v["peak"] = max(v["peak"], len(nxt))
        sets.append(nxt)
        cur = nxt
    v.update(verdict="accepted", step=len(observations))
    return v, sets


def paths(g, length, limit=None):
    """every path of exactly `length` states from an initial state through steps a behaviour may take (unflagged successors, in the
    model or not; a state the graph did not expand ends its paths), as tuples of texts, in a fixed order; at most `limit`"""
    out = []
    todo = [(e.text,) for e in reversed(list(dict.fromkeys(g.init)))]
    seen_init = set()
    while todo:
        p = todo.pop()
        if len(p) == 1:
            if p[0] in seen_init:
                continue
            seen_init.add(p[0])
        if len(p) == length:
            out.append(p)
            if limit and len(out) >= limit:
                break
            continue
        nxt = list(dict.fromkeys(e.text for e in g.succ.get(p[-1], ()) if not e.flags & (F_ASSERT | F_SPECERR)))
        for t in reversed(nxt):
            todo.append(p + (t,))
    return out
