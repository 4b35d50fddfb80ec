"""A plain reference for cfg VIEW and ACTION_CONSTRAINT on compiled PlusCal programs, with no engine code involved:
oracle/tla_eval.py's Checker over Program.translated(), with two definitions appended —

    CfgAcNext == Next /\\ A1 /\\ A2 ...     ck.successors(s, nxt="CfgAcNext") are the ALLOWED steps of s
    CfgView == <<...>>                      evaluated per state

— and a breadth-first search written here.  The rules are restated from TLC's manual, not from the product:

    a successor is generated (and counted) whether or not its transition is allowed; it is invariant-checked either way;
    it is stored — and later expanded — only if the transition satisfies every action constraint, the state every CONSTRAINT, and no
    state with the same VIEW value has been stored before (initial states included);
    a state without any generated successor is a deadlock.

The representative of a view value is free (the first to arrive), so engines are compared by the SETS OF VIEW VALUES per level
(view_of_text() evaluates CfgView on a state the engine printed)."""
import re
import sys
from collections import namedtuple

import helpers

sys.path.insert(0, str(helpers.ROOT / "oracle"))

DIR = helpers.ROOT / "specs_cfgmore"

# name -> what the model was WRITTEN to show, as facts about the reference's result (test_cfgmore_host.py checks them before anything
# relies on the reference): distinct states, depth, verdict; congruent: the view is a congruence (equal views, equal futures)
Model = namedtuple("Model", "distinct depth verdict congruent")
MODELS = {
    "ghost_history": Model(150, 16, "ok", True),
    "ghost_unbounded": Model(150, 16, "ok", True),
    "parity_view": Model(16, 6, "deadlock", True),
    "view_init": Model(13, 5, "ok", True),
    "ac_monotone": Model(6, 3, "ok", False),
    "ac_indexed": Model(100, 19, "ok", False),
    "ac_two": Model(5, 2, "invariant", False),
    "ac_deadlock": Model(2, 2, "ok", False),
    "ac_deadlock_twin": Model(2, 2, "ok", False),
    "ac_records": Model(288, 7, "ok", False),
    "wide": Model(1225, 9, "ok", True),
    "view_kinds": Model(20, 7, "ok", True),
    "ac_soup": Model(569, 7, "ok", False),
}
# file -> the word its refusal must contain
REFUSED = {"refuse_prime": "prime", "refuse_view": "{y, 1}", "refuse_unknown": "Nope", "refuse_nonbool": "Boolean", "refuse_symmetry": "SYMMETRY",
           "refuse_primed_quant": "quantifier over the primed set of records `msgs'`", "refuse_primed_seq": "a primed sequence can be compared with a tuple of constants only"}


def texts(name):
    return (DIR / f"{name}.tla").read_text(), (DIR / f"{name}.cfg").read_text()


def read_cfg(text):
    """the statements of a cfg this reference knows: {keyword: [names]} and the constants"""
    plural = {"INVARIANT": "INVARIANT", "INVARIANTS": "INVARIANT", "CONSTRAINT": "CONSTRAINT", "CONSTRAINTS": "CONSTRAINT",
              "ACTION_CONSTRAINT": "ACTION_CONSTRAINT", "ACTION_CONSTRAINTS": "ACTION_CONSTRAINT", "ACTION-CONSTRAINT": "ACTION_CONSTRAINT",
              "PROPERTY": "PROPERTY", "VIEW": "VIEW", "SPECIFICATION": "SPECIFICATION", "CONSTANT": "CONSTANT", "CONSTANTS": "CONSTANT"}
    out = {k: [] for k in set(plural.values())}
    consts, key = {}, None
    toks = text.replace("=", " = ").split()
    i = 0
    while i < len(toks):
        t = toks[i]
        if t in plural:
            key = plural[t]
        elif key == "CONSTANT":
            assert toks[i + 1] == "="
            consts[t] = int(toks[i + 2])
            i += 2
        else:
            out[key].append(t)
        i += 1
    out["CONSTANT"] = consts
    return out


class Reference:
    def __init__(self, program, cfg_text, with_view=True, with_acons=True, extra_constraints=()):
        from tla_eval import Checker
        cfg = read_cfg(cfg_text)
        self.acons = cfg["ACTION_CONSTRAINT"] if with_acons else []
        self.view = cfg["VIEW"][0] if cfg["VIEW"] and with_view else None
        self.invariants, self.constraints = cfg["INVARIANT"], cfg["CONSTRAINT"] + list(extra_constraints)
        text = program.translated()
        # the translation keeps a record variable r field by field and DEFINES r == [f |-> r_f, ...]; the evaluator primes variables only, so
        # the primed record is given to it as what it means: r'.f = r_f', r' = [f |-> r_f', ...], UNCHANGED r = UNCHANGED <<r_f, ...>>
        for rec, body in re.findall(r"^(\w+) == (\[\w+ \|-> \1_\w+.*\])$", text, flags=re.M):
            fields = re.findall(rf"\b{rec}_\w+", body)
            text = re.sub(rf"\b{rec}'\.(\w+)", rf"{rec}_\1'", text)
            text = re.sub(rf"\bUNCHANGED {rec}\b", "UNCHANGED <<" + ", ".join(fields) + ">>", text)
            text = re.sub(rf"\b{rec}'", "(" + re.sub(rf"\b({rec}_\w+)", r"\1'", body).replace("\\", "\\\\") + ")", text)
        extra = "CfgAcNext == Next" + "".join(f" /\\ {a}" for a in self.acons) + "\n"
        extra += f"CfgView == {self.view}\n" if self.view else ""
        at = text.rindex("\n====") + 1   # the module's closing line
        self.ck = Checker(text[:at] + extra + text[at:], constants=dict(cfg["CONSTANT"]))
        self.ck.engine_mode = True   # a failing Assert is one generated successor

    def line(self, s):
        return self.ck.fmt_state(s).replace("\n", " ")

    def view_of(self, s):
        """the view value of a state (hashable), or the whole state without a VIEW"""
        ck = self.ck
        return ck.ev(ck.defs["CfgView"][1], s, None, {}) if self.view else ck.key(s)

    def state_of_text(self, text):
        """a state as an engine prints it: `/\\ x = 0 /\\ pc = <<"a", "b">> ...` (one line or several)"""
        from tla_eval import Parser, lex
        ck = self.ck
        parts = [p.strip() for p in text.replace("\n", " ").split("/\\ ") if p.strip()]
        s = {}
        for p in parts:
            var, _, val = p.partition(" = ")
            s[var.strip()] = ck.ev(Parser(lex(val)).expr(), {}, None, {})
        assert set(s) == set(ck.vars), (text, ck.vars)
        return s

    def view_of_text(self, text):
        return self.view_of(self.state_of_text(text))

    def steps(self, s):
        """every generated successor of s as (state, allowed)"""
        ck = self.ck
        allowed = {}
        for n in ck.successors(s, nxt="CfgAcNext"):
            if "__assert__" not in n:
                allowed[ck.key(n)] = 1
        for n in ck.successors(s, nxt="Next"):
            yield n, "__assert__" not in n and ck.key(n) in allowed

    def run(self, check_deadlock=True):
        """-> dict(distinct, generated, depth, verdict, trace_len, levels, level_views (one set of view values per level), level_lines,
        edges (the allowed steps between stored states, by line; only meaningful without a view))"""
        ck = self.ck
        res = dict(distinct=0, generated=0, depth=0, verdict="ok", violated=None, trace_len=0, levels=[], level_views=[], level_lines=[], edges=set(),
                   refused=0)
        seen = set()

        def bad_inv(s):
            for name in self.invariants:
                if not ck.ev(ck.defs[name][1], s, None, {}):
                    return name
            return None

        def fail(verdict, violated, trace_len):
            if res["verdict"] == "ok":
                res.update(verdict=verdict, violated=violated, trace_len=trace_len)
        cur = []
        for s in ck.initial_states():
            res["generated"] += 1
            if bad_inv(s):
                fail("invariant", bad_inv(s), 1)
            if not ck.in_model(s, self.constraints):
                continue
            v = self.view_of(s)
            if v not in seen:
                seen.add(v)
                cur.append(s)
        level = 1
        while cur:
            res["levels"].append(len(cur))
            res["level_views"].append({self.view_of(s) for s in cur})
            res["level_lines"].append(sorted(self.line(s) for s in cur))
            if res["verdict"] != "ok":
                break
            nxt = []
            for s in cur:
                nsucc = 0
                for n, allowed in self.steps(s):
                    nsucc += 1
                    res["generated"] += 1
                    if "__assert__" in n:
                        fail("assert", None, level)
                        continue
                    if bad_inv(n):
                        fail("invariant", bad_inv(n), level + 1)
                    if not allowed:
                        res["refused"] += 1
                        continue
                    if not ck.in_model(n, self.constraints):
                        continue
                    res["edges"].add((self.line(s), self.line(n)))
                    v = self.view_of(n)
                    if v not in seen:
                        seen.add(v)
                        nxt.append(n)
                if nsucc == 0 and check_deadlock:
                    fail("deadlock", None, level)
            cur = nxt
            if cur:
                level += 1
        if res["verdict"] != "ok" and cur and len(res["levels"]) < level:
            res["levels"].append(len(cur))
            res["level_views"].append({self.view_of(s) for s in cur})
            res["level_lines"].append(sorted(self.line(s) for s in cur))
        res.update(distinct=len(seen), depth=level)
        return res


_cache = {}


def compiled(name):
    import tla_rust_amd as amd
    tla, cfg = texts(name)
    return amd.Program(tla, cfg)


def load(name):
    """(program, reference, the reference's result) of a model; computed once and shared — nobody changes it"""
    if name not in _cache:
        prog = compiled(name)
        ref = Reference(prog, texts(name)[1])
        _cache[name] = (prog, ref, ref.run())
    return _cache[name]


def level_views_of_dump(ref, path):
    """a dump file of state texts (`L<level> <state>` per line) -> one set of view values per level"""
    out = []
    for ln in open(path).read().splitlines():
        lv, _, text = ln.partition(" ")
        k = int(lv[1:])
        while len(out) < k:
            out.append(set())
        out[k - 1].add(ref.view_of_text(text))
    return out


def sim_graph(ref):
    """the reference's graph in tests/simgraph.py's form: a REFUSED transition is an edge that is generated and cannot be walked, exactly
    as an edge to a successor outside a CONSTRAINT (inmodel = False)"""
    import simgraph
    ck = ref.ck

    def edge(s, allowed, action=0):
        if "__assert__" in s:
            return simgraph.Edge("-", False, -1, simgraph.F_ASSERT, action)
        inv = next((k for k, name in enumerate(ref.invariants) if not ck.ev(ck.defs[name][1], s, None, {})), -1)
        return simgraph.Edge(ref.line(s), bool(allowed and ck.in_model(s, ref.constraints)), inv, 0, action)
    init, succ, todo = [], {}, []
    for s in ck.initial_states():
        init.append(edge(s, True, -1))
        todo.append((init[-1], s))
    while todo:
        e, st = todo.pop()
        if not e.inmodel or e.text in succ:
            continue
        out = succ[e.text] = []
        for n, allowed in ref.steps(st):
            out.append(edge(n, allowed))
            if "__assert__" not in n:
                todo.append((out[-1], n))
    return simgraph.Graph(init, succ)


def gen_check(prog):
    """tests/_cfgmore/harness_cfg.cpp built around the generated code of `prog` (g++, cached by the hash of everything it is made of):
    generated code against the interpreter with the cfg's statements on every reachable state and slot (helpers.gen_check's route)"""
    import ctypes as C
    import hashlib

    import testlib

    class Handle:
        h = prog.params[0]
    root, csrc = helpers.ROOT, helpers.ROOT / "tla_rust_amd" / "csrc"
    text = helpers.program_codegen(Handle)
    srcs = [root / "tests" / "_cfgmore" / "harness_cfg.cpp", root / "tests" / "_gen" / "harness.cpp", csrc / "spec_gen.h", csrc / "spec_vm.h", csrc / "spec_vm_cfg.h"]
    tag = hashlib.sha256((text + "".join(s.read_text() for s in srcs)).encode()).hexdigest()[:16]
    out = root / "tests" / "_cfgmore" / "_build"
    so = testlib.build_generated(out / f"libgen_{tag}.so", out / f"gen_{tag}.h", text, [srcs[0]])
    C.CDLL(str(helpers.build_shim()), mode=C.RTLD_GLOBAL)   # the interpreter's host helpers (vm_make_params, ...) live in the front-end
    lib = C.CDLL(str(so))
    lib.gen_check.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(helpers.GenCheck)]
    r = helpers.GenCheck()
    rc = lib.gen_check(Handle.h, 0, C.byref(r))
    assert rc == 0, rc
    return {k: getattr(r, k) for k, _ in helpers.GenCheck._fields_}
