"""The reference for liveness under fairness label by label on the models of specs_labelfair/ (DESIGN.md section 21), with no engine
code involved: tests/liveprops.py's PropGraph (the state graph of the module under oracle/tla_eval.py, the predicates' bits) plus,
for every fairness CONJUNCT of the translation's Spec, the steps that satisfy its action — one definition LiveC_k == <the action inside
WF_vars( ) / SF_vars( )> is appended to the translation, as LiveP_k is, and ck.successors(state, nxt="LiveC_k") gives the steps.  The
conjuncts' texts are the product's (Program.fairness_units; tests/test_labelfair_host.py pins them to the hand-written EXPECT below);
whether a conjunct is weak or strong is read off its text.  The rule is tests/unitfair.decide_units: a unit of the reference is a set of
conjuncts — the conjuncts that have a step i -> j — so the two sides share the program text alone."""
import sys

import helpers
import liveprops
import strongfair
import unitfair

sys.path.insert(0, str(helpers.ROOT / "oracle"))

DIR = helpers.ROOT / "specs_labelfair"
Model = liveprops.Model   # tla cfg constants procs expect

# name -> (module, cfg, constants, the process instances' actions in slot order, {check name: is it violated under pcal2tla's fairness?})
MODELS = {
    "lock_plus": Model("lock_plus.tla", "lock_plus.cfg", {}, ["P(0)", "P(1)"], {"Served[i = 0]": False, "Served[i = 1]": False}),
    "lock_weak": Model("lock_weak.tla", "lock_weak.cfg", {}, ["P(0)", "P(1)"], {"Served[i = 0]": True, "Served[i = 1]": True}),
    "spin_minus": Model("spin_minus.tla", "spin_minus.cfg", {}, ["Spinner", "Setter"], {"Termination": True}),
    "spin_fair": Model("spin_fair.tla", "spin_fair.cfg", {}, ["Spinner", "Setter"], {"Termination": False}),
    "two_labels_minus": Model("two_labels_minus.tla", "two_labels_minus.cfg", {}, ["Spinner", "Setter"], {"Termination": True}),
    "toggle_plus": Model("toggle_plus.tla", "toggle_plus.cfg", {}, ["Waiter", "Toggler"], {"Termination": False}),
    "fairplus_plus": Model("fairplus_plus.tla", "fairplus_plus.cfg", {}, ["Waiter", "Toggler"], {"Termination": False}),
    "fairplus_plain": Model("fairplus_plain.tla", "fairplus_plain.cfg", {}, ["Waiter", "Toggler"], {"Termination": False}),
    "unfair_plus": Model("unfair_plus.tla", "unfair_plus.cfg", {}, ["Waiter", "Toggler"], {"Termination": True}),
    # procedures: a conjunct of the process's own labels and one per procedure it reaches
    "treiber_procs": Model("treiber_procs.tla", "treiber_procs.cfg", {}, ["Pusher", "Popper"], {"PushDone": False}),
    "lock_proc": Model("lock_proc.tla", "lock_proc.cfg", {}, ["P(0)", "P(1)"], {"Served[i = 0]": False, "Served[i = 1]": False}),
    "proc_minus": Model("proc_minus.tla", "proc_minus.cfg", {}, ["Caller"], {"Termination": True}),
    "rec_fair": Model("rec_fair.tla", "rec_fair.cfg", {}, ["Walker"], {"Termination": False}),
}
# the fairness conjuncts of Spec as the translation must print them, and per instance (Program.fairness_units' texts, in its order)
EXPECT = {
    "lock_plus": (["\\A self \\in {0, 1} : WF_vars(P(self))", "\\A self \\in {0, 1} : SF_vars(wait(self))"],
                  ["WF_vars(P(0))", "SF_vars(wait(0))", "WF_vars(P(1))", "SF_vars(wait(1))"]),
    "lock_weak": (["\\A self \\in {0, 1} : WF_vars(P(self))"], ["WF_vars(P(0))", "WF_vars(P(1))"]),
    "spin_minus": (['WF_vars((pc[0] \\notin {"spin"}) /\\ Spinner)', "WF_vars(Setter)"], ['WF_vars((pc[0] \\notin {"spin"}) /\\ Spinner)', "WF_vars(Setter)"]),
    "spin_fair": (["WF_vars(Spinner)", "WF_vars(Setter)"], ["WF_vars(Spinner)", "WF_vars(Setter)"]),
    "two_labels_minus": (["WF_vars(Spinner)", 'WF_vars((pc[1] \\notin {"idle"}) /\\ Setter)'], ["WF_vars(Spinner)", 'WF_vars((pc[1] \\notin {"idle"}) /\\ Setter)']),
    "toggle_plus": (["WF_vars(Waiter)", "SF_vars(W)", "WF_vars(Toggler)"], ["WF_vars(Waiter)", "SF_vars(W)", "WF_vars(Toggler)"]),
    "fairplus_plus": (["SF_vars(Waiter)", "WF_vars(Toggler)"], ["SF_vars(Waiter)", "WF_vars(Toggler)"]),
    "fairplus_plain": (["SF_vars(Waiter)", "WF_vars(Toggler)"], ["SF_vars(Waiter)", "WF_vars(Toggler)"]),
    "unfair_plus": (["WF_vars(Toggler)"], ["WF_vars(Toggler)"]),
    "treiber_procs": (["WF_vars(go \\/ fin)", "WF_vars(rd_p1 \\/ cas_p1)"], ["WF_vars(go \\/ fin)", "WF_vars(rd_p1 \\/ cas_p1)"]),
    "lock_proc": (["\\A self \\in {0, 1} : WF_vars(ncs(self) \\/ cs(self))", "\\A self \\in {0, 1} : WF_vars(wait_p1(self))", "\\A self \\in {0, 1} : SF_vars(wait_p1(self))"],
                  ["WF_vars(ncs(0) \\/ cs(0))", "WF_vars(wait_p1(0))", "SF_vars(wait_p1(0))", "WF_vars(ncs(1) \\/ cs(1))", "WF_vars(wait_p1(1))", "SF_vars(wait_p1(1))"]),
    "proc_minus": (["WF_vars(c \\/ d)", 'WF_vars((pc[0] \\notin {"rest_p1"}) /\\ (in_p1 \\/ rest_p1))'],
                   ["WF_vars(c \\/ d)", 'WF_vars((pc[0] \\notin {"rest_p1"}) /\\ (in_p1 \\/ rest_p1))']),
    "rec_fair": (["WF_vars(w \\/ e)", "WF_vars(d1_p1 \\/ d2_p1)"], ["WF_vars(w \\/ e)", "WF_vars(d1_p1 \\/ d2_p1)"]),
    "uni_minus": (['WF_vars((pc \\notin {"b"}) /\\ Next)'], ['WF_vars((pc \\notin {"b"}) /\\ Next)']),
}


def compiled(stem):
    import tla_rust_amd as amd
    return amd.Program((DIR / (stem + ".tla")).read_text(), (DIR / (stem + ".cfg")).read_text())


def spec_conjuncts(translation):
    """the fairness conjuncts of Spec in a translation's text, one per `/\\` line after the first"""
    spec = translation[translation.index("\nSpec =="):]
    spec = spec[:spec.index("\n\n")]
    return [ln.strip()[3:].strip() for ln in spec.splitlines()[2:]]


def action_of(conjunct):
    assert conjunct[:8] in ("WF_vars(", "SF_vars(") and conjunct.endswith(")"), conjunct
    return conjunct[8:-1]


class UnitGraph(liveprops.PropGraph):
    """PropGraph plus conj[i][k] = the states a step of conjunct k leads to from state i, and the reference's own units: uedges[i] =
    [(unit or -1, j)] over the process edges, of_unit[u] = the conjuncts with a step i -> j (a set), weak / strong from the texts"""

    def __init__(self, program, model, conjuncts):
        super().__init__(program, model)
        from tla_eval import Checker
        text = program.translated()
        extra = "".join(f"LiveC_{k} == {action_of(c)}\n" for k, c in enumerate(conjuncts))
        at = text.rindex("\n====") + 1
        ck = Checker(text[:at] + extra + text[at:], constants=dict(model.constants))

        def line(s):
            return ck.fmt_state(s).replace("\n", " ")
        self.nconj = len(conjuncts)
        self.weak = sum(1 << k for k, c in enumerate(conjuncts) if c.startswith("WF_"))
        self.strong = sum(1 << k for k, c in enumerate(conjuncts) if c.startswith("SF_"))
        self.conj = [None] * len(self.texts)
        todo = list(ck.initial_states())
        while todo:
            s = todo.pop()
            i = self.index[line(s)]
            if self.conj[i] is not None:
                continue
            self.conj[i] = [{self.index[line(n)] for n in ck.successors(s, nxt=f"LiveC_{k}")} for k in range(self.nconj)]
            todo.extend(ck.successors(s))
        assert all(c is not None for c in self.conj)
        ids, self.of_unit, self.uedges = {}, [], []
        for i, row in enumerate(self.edges):
            out = []
            for p, j in row:
                if p < 0:
                    out.append((-1, j))
                    continue
                key = frozenset(k for k in range(self.nconj) if j in self.conj[i][k])
                if key not in ids:
                    ids[key] = len(self.of_unit)
                    self.of_unit.append(set(key))
                out.append((ids[key], j))
            self.uedges.append(out)

    def members(self, i, j):
        """the conjuncts with a step i -> j"""
        return {k for k in range(self.nconj) if j in self.conj[i][k]}


def load(name):
    """(Program, UnitGraph, the checks of its cfg) of a model of MODELS; the caller closes the program"""
    m = MODELS[name]
    prog = compiled(m.tla[:-4])
    fu, texts, why = prog.fairness_units
    assert why is None, why
    return prog, UnitGraph(prog, m, texts), strongfair.checks_of(prog, (DIR / m.cfg).read_text())


def decide_model(g, prop, rank=None):
    return unitfair.decide_units(g.uedges, g.of_unit, g.nconj, len(g.init), g.bits, g.done, prop, g.weak, g.strong, rank)
