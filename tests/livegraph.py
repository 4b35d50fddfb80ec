"""A plain reference for `Termination` under weak process fairness, with no engine code involved: the state graph of a PlusCal module
under oracle/tla_eval.py's Checker over Program.translated(), with one definition appended per process instance (LiveP_k == p(k)), so
that ck.successors(state, nxt="LiveP_k") gives the steps of instance k.  States are identified by their one-line text, as
tests/simgraph.py does.  The rule is restated from DESIGN.md section 16, not from liveness.h:

    en(s, p)      s has a step of p to a DIFFERENT state
    taken(C)      the p with a step u -> v, u # v, u and v in the strongly connected component C
    disabled(C)   the p with ~en(s, p) for some s in C
    C is fair     iff every fair p is in taken(C) or disabled(C);  Termination is violated iff some fair C holds no Done state

Components come from an iterative Tarjan (tarjan() below, also used on the engine's arrays by tests/test_gpu_liveness.py)."""
import sys
from collections import namedtuple

import helpers

sys.path.insert(0, str(helpers.ROOT / "oracle"))

DIR = helpers.ROOT / "specs_liveness"

# name -> (module file, cfg file, constants, the process instances' actions in ascending identifier order (the engine's slot order),
#          is Termination violated?)   — the last column is what the models were WRITTEN to show; test_liveness_host.py checks the
# reference against it before anything relies on the reference
Model = namedtuple("Model", "tla cfg constants procs violated")
MODELS = {
    "handoff": Model("handoff.tla", "handoff.cfg", {}, ["P(0)", "P(1)", "P(2)"], False),
    "handoff_unfair": Model("handoff_unfair.tla", "handoff_unfair.cfg", {}, ["P(0)", "P(1)", "P(2)"], True),
    "spin_flag": Model("spin_flag.tla", "spin_flag.cfg", {}, ["Spinner", "Setter"], False),
    "spin_flag_unfair": Model("spin_flag_unfair.tla", "spin_flag_unfair.cfg", {}, ["Spinner", "Setter"], True),
    "starve_wf": Model("starve_wf.tla", "starve_wf.cfg", {}, ["Waiter", "Flipper"], True),
    "self_step": Model("self_step.tla", "self_step.cfg", {}, ["Idle", "Peer"], True),
    "self_step_exit": Model("self_step_exit.tla", "self_step_exit.cfg", {}, ["Dither"], False),
    "ring": Model("ring.tla", "ring.cfg", {"N": 65}, ["Counter", "Stopper"], True),
    "two_loops": Model("two_loops.tla", "two_loops.cfg", {}, ["Toggler", "Switch", "Fin"], True),
}
REFUSED = {"refused_strong": "fair+", "refused_label": "modifier", "refused_procedure": "procedures"}


def tarjan(n, succ):
    """components of the graph on 0 .. n-1 (succ(v): iterable of successors) as comp[v] = the LEAST vertex of v's component; iterative"""
    index, low, comp = [-1] * n, [0] * n, [-1] * n
    on, stack, count = [False] * n, [], 0
    for root in range(n):
        if index[root] >= 0:
            continue
        work = [(root, iter(succ(root)))]
        index[root] = low[root] = count
        count += 1
        stack.append(root)
        on[root] = True
        while work:
            v, it = work[-1]
            advanced = False
            for w in it:
                if index[w] < 0:
                    index[w] = low[w] = count
                    count += 1
                    stack.append(w)
                    on[w] = True
                    work.append((w, iter(succ(w))))
                    advanced = True
                    break
                if on[w]:
                    low[v] = min(low[v], index[w])
            if advanced:
                continue
            work.pop()
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
            if low[v] == index[v]:
                members = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    members.append(w)
                    if w == v:
                        break
                least = min(members)
                for w in members:
                    comp[w] = least
    return comp


class LiveGraph:
    """texts: the states in discovery order; index: text -> number; edges[i] = [(process or -1 for the terminating disjunct, j)];
    init: the initial states' numbers; done[i]; en[i] = set of processes with a real step"""

    def __init__(self, program, model):
        from tla_eval import Checker
        text = program.translated()
        extra = "".join(f"LiveP_{k} == {a}\n" for k, a in enumerate(model.procs)) + 'LiveDone == \\A self \\in ProcSet: pc[self] = "Done"\n'
        at = text.rindex("\n====") + 1   # the module's closing line
        ck = Checker(text[:at] + extra + text[at:], constants=dict(model.constants))
        self.nproc = len(model.procs)

        def line(s):
            return ck.fmt_state(s).replace("\n", " ")
        self.texts, self.index, states = [], {}, []
        for s in ck.initial_states():
            t = line(s)
            if t not in self.index:
                self.index[t] = len(self.texts)
                self.texts.append(t)
                states.append(s)
        self.init = list(range(len(self.texts)))
        self.edges, self.done, self.en = [], [], []
        i = 0
        while i < len(states):
            s = states[i]
            out, en = [], set()
            for k in range(self.nproc):
                for n in ck.successors(s, nxt=f"LiveP_{k}"):
                    t = line(n)
                    if t not in self.index:
                        self.index[t] = len(self.texts)
                        self.texts.append(t)
                        states.append(n)
                    out.append((k, self.index[t]))
                    if self.index[t] != i:
                        en.add(k)
            done = bool(ck.ev(ck.defs["LiveDone"][1], s, None, {}))
            if done:
                out.append((-1, i))
            self.edges.append(out)
            self.done.append(done)
            self.en.append(en)
            i += 1
        self.comp = tarjan(len(self.texts), lambda v: [j for _, j in self.edges[v]])

    def components(self):
        """{component id: (members, taken, disabled, holds a Done state)}"""
        out = {}
        for v, c in enumerate(self.comp):
            m, taken, disabled, done = out.setdefault(c, ([], set(), set(), [False]))
            m.append(v)
            done[0] |= self.done[v]
            disabled |= set(range(self.nproc)) - self.en[v]
            taken |= {p for p, j in self.edges[v] if p >= 0 and j != v and self.comp[j] == c}
        return {c: (m, t, d, dn[0]) for c, (m, t, d, dn) in out.items()}

    def fair_components(self, fair_mask):
        """the components (as frozensets of state texts) that are fair under the mask and hold no Done state"""
        fair = {p for p in range(self.nproc) if fair_mask >> p & 1}
        return [frozenset(self.texts[v] for v in m) for m, t, d, dn in self.components().values() if not dn and fair <= (t | d)]

    def partition(self):
        """the components as a set of frozensets of state texts"""
        return {frozenset(self.texts[v] for v in m) for m, _, _, _ in self.components().values()}


def load(name):
    """(Program, LiveGraph) of a model of MODELS; the caller closes the program"""
    import tla_rust_amd as amd
    m = MODELS[name]
    prog = amd.Program((DIR / m.tla).read_text(), (DIR / m.cfg).read_text())
    return prog, LiveGraph(prog, m)
