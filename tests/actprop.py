"""A plain reference for the SAFETY parts of a cfg PROPERTY on compiled PlusCal programs, with no engine code involved:
oracle/tla_eval.py's Checker over Program.translated(), with the conjuncts of every named property appended as plain definitions —

    `[][A]_v`   ->  RefA_k == A,  RefV_k == v     checked on every GENERATED successor n of s: ck.ev(A, s, n) or v unchanged
    `[]P`       ->  RefP_k == P                   checked on every generated state, as an INVARIANT is
    `I`         ->  RefI_k == I                   checked on the initial states
    WF_ / SF_, <>, ~>                             liveness: not this reference's business (listed in `live`)

— and a breadth-first search written here, on top of tests/cfgmore.py's (its Reference reads the cfg, rewrites primed records and tells
which steps an ACTION_CONSTRAINT refuses).  The rule is TLC's doNextCheckImplied, restated: every generated successor is checked, new or
not, refused or outside a CONSTRAINT or not; a successor that breaks an INVARIANT as well reports the invariant; the engine's convention
that a level is finished before the search stops is kept, and within a level the first violation in the order (state, successor) counts."""
import re
from collections import namedtuple

import cfgmore
import helpers

DIR = helpers.ROOT / "specs_actprop"

# cfg -> what the model was WRITTEN to show, as facts about the reference's result: verdict, the violated PROPERTY / INVARIANT, the length of
# the behaviour, distinct states (None: not pinned)
Model = namedtuple("Model", "verdict violated trace_len distinct")
MODELS = {
    "ap_monotone": Model("invariant", "Mono", 2, None),
    "ap_monotone_ok": Model("ok", None, 0, 25),
    "ap_seen": Model("invariant", "Up", 4, 3),
    "ap_subscript": Model("ok", None, 0, None),
    "ap_subscript_tuple": Model("invariant", "IncXY", 2, None),
    "ap_done": Model("ok", None, 0, 3),
    "ap_spec": Model("ok", None, 0, 5),
    "ap_spec_badstep": Model("invariant", "HSpecStrict", 5, None),
    "ap_spec_badinit": Model("invariant", "HSpecOne", 1, None),
    "ap_always": Model("invariant", "Small", 5, None),
    "ap_kinds": Model("ok", None, 0, None),
    "ap_kinds_bad": Model("invariant", "KBad", 2, None),
    "ap_soup": Model("ok", None, 0, None),
    "ap_soup_bad": Model("invariant", "AtMostOne", 3, None),
    "ap_refused_step": Model("invariant", "Mono", 2, None),
    "ap_mixed": Model("ok", None, 0, 4),
    "ap_two": Model("invariant", "Inv", 2, None),
}
# file -> the word its refusal must contain
REFUSED = {"refuse_angle": "<<A>>_v", "refuse_form": "a primed sequence / set of records / function can be compared with", "refuse_next": "Next",
           "refuse_subscript": "subscript", "refuse_many": "at most 8 action properties"}


def texts(name):
    """(module text, cfg text): a cfg without a module of its own name belongs to the module whose name it starts with"""
    tla = DIR / f"{name}.tla"
    if not tla.exists():
        tla = max((t for t in DIR.glob("*.tla") if name.startswith(t.stem)), key=lambda t: len(t.stem))
    return tla.read_text(), (DIR / f"{name}.cfg").read_text()


def split_top(body, sep):
    """the pieces of `body` between the occurrences of `sep` outside every bracket"""
    out, depth, start, i = [], 0, 0, 0
    while i < len(body):
        if body.startswith(("<<", ">>"), i):
            depth += 1 if body[i] == "<" else -1
            i += 2
            continue
        if body[i] in "([{":
            depth += 1
        elif body[i] in ")]}":
            depth -= 1
        elif depth == 0 and body.startswith(sep, i):
            out.append(body[start:i].strip())
            start = i + len(sep)
            i = start
            continue
        i += 1
    out.append(body[start:].strip())
    return [p for p in out if p]


def conjuncts(module_text, name):
    """the definition `name` of the module text as (kind, A or P or I, v or None, text) per conjunct; kind: step / always / init / live"""
    m = re.search(rf"^{name} == (.*)$", module_text, flags=re.M)
    assert m, name
    out = []
    for c in split_top(m.group(1), "/\\"):
        if c.startswith("[]["):
            depth, i = 0, 2
            while True:
                depth += {"[": 1, "]": -1}.get(c[i], 0)
                if depth == 0:
                    break
                i += 1
            assert c[i + 1] == "_", c
            out.append(("step", c[3:i], c[i + 2:], c))
        elif c.startswith("[]") and not c.startswith("[]<>"):
            out.append(("always", c[2:], None, c))
        elif c.startswith(("WF_", "SF_")) or "~>" in c or "<>" in c:
            out.append(("live", c, None, c))
        else:
            out.append(("init", c, None, c))
    return out


class Reference(cfgmore.Reference):
    def __init__(self, program, module_text, cfg_text, with_properties=True):
        self.props = []   # (PROPERTY, kind, definition of A / P / I, definition of v or None)
        self.live = []    # (PROPERTY, conjunct): the liveness parts
        extra = ""
        cfg = cfgmore.read_cfg(cfg_text)
        for name in cfg["PROPERTY"] if with_properties else []:
            for k, (kind, a, v, text) in enumerate(conjuncts(module_text, name)):
                if kind == "live":
                    self.live.append((name, text))
                    continue
                extra += f"Ref{name}{k}A == {a}\n" + (f"Ref{name}{k}V == {v}\n" if v else "")
                self.props.append((name, kind, f"Ref{name}{k}A", f"Ref{name}{k}V" if v else None))
        self._extra = extra
        translated = program.translated

        class WithExtra:   # (cfgmore.Reference reads the text once, from program.translated(): the definitions go in before the closing line)
            def translated(self):
                text = translated()
                at = text.rindex("\n====") + 1
                return text[:at] + extra + text[at:]
        super().__init__(WithExtra(), cfg_text, with_view=False)

    def bad_step(self, s, n):
        """the first `[][A]_v` the step s -> n breaks, or None"""
        ck = self.ck
        for name, kind, a, v in self.props:
            if kind != "step":
                continue
            if ck.ev(ck.defs[v][1], s, None, {}) == ck.ev(ck.defs[v][1], n, None, {}):
                continue
            if not ck.ev(ck.defs[a][1], s, n, {}):
                return name
        return None

    def bad_state(self, s, initial):
        """the first INVARIANT, `[]P` or (on an initial state) initial predicate the state breaks, or None"""
        ck = self.ck
        for name in self.invariants:
            if not ck.ev(ck.defs[name][1], s, None, {}):
                return name
        for kinds in (("always",), ("init",) if initial else ()):
            for name, kind, a, _ in self.props:
                if kind in kinds and not ck.ev(ck.defs[a][1], s, None, {}):
                    return name
        return None

    def run(self, check_deadlock=True):
        """-> dict(distinct, generated, depth, verdict, violated, trace_len, last_step (the lines of the offending step, or None), levels,
        level_lines, step_violations (per PROPERTY: the violating steps of the levels searched), state_violations)"""
        ck = self.ck
        res = dict(distinct=0, generated=0, depth=0, verdict="ok", violated=None, trace_len=0, last_step=None, levels=[], level_lines=[],
                   step_violations={}, state_violations={})
        seen = set()

        def fail(verdict, violated, trace_len, last_step=None):
            if res["verdict"] == "ok":
                res.update(verdict=verdict, violated=violated, trace_len=trace_len, last_step=last_step)
        cur = []
        for s in ck.initial_states():
            res["generated"] += 1
            bad = self.bad_state(s, True)
            if bad:
                res["state_violations"].setdefault(bad, set()).add(self.line(s))
                fail("invariant", bad, 1)
            if not ck.in_model(s, self.constraints):
                continue
            if ck.key(s) not in seen:
                seen.add(ck.key(s))
                cur.append(s)
        level = 1
        while cur:
            res["levels"].append(len(cur))
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
                    bad = self.bad_state(n, False)
                    if bad:   # (the status word carries one index: the invariant's)
                        res["state_violations"].setdefault(bad, set()).add(self.line(n))
                        fail("invariant", bad, level + 1)
                    step = self.bad_step(s, n)
                    if step:
                        res["step_violations"].setdefault(step, set()).add((self.line(s), self.line(n)))
                        if not bad:
                            fail("invariant", step, level + 1, (self.line(s), self.line(n)))
                    if not allowed or not ck.in_model(n, self.constraints):
                        continue
                    if ck.key(n) not in seen:
                        seen.add(ck.key(n))
                        nxt.append(n)
                if nsucc == 0 and check_deadlock:
                    fail("deadlock", None, level)
            cur = nxt
            if cur:
                level += 1
        if res["verdict"] != "ok" and cur and len(res["levels"]) < level:
            res["levels"].append(len(cur))
            res["level_lines"].append(sorted(self.line(s) for s in cur))
        res.update(distinct=len(seen), depth=level)
        return res

    def breaks(self, name, before, after):
        """does the step between two states, given as an engine prints them, break the `[][A]_v` conjuncts of PROPERTY `name`?"""
        s, n = self.state_of_text(before), self.state_of_text(after)
        ck = self.ck
        return any(p == name and kind == "step" and ck.ev(ck.defs[v][1], s, None, {}) != ck.ev(ck.defs[v][1], n, None, {}) and
                   not ck.ev(ck.defs[a][1], s, n, {}) for p, kind, a, v in self.props)


_cache = {}


def compiled(name):
    import tla_rust_amd as amd
    return amd.Program(*texts(name))


def load(name):
    """(program, reference, the reference's result) of a cfg; computed once and shared — nobody changes it"""
    if name not in _cache:
        prog = compiled(name)
        tla, cfg = texts(name)
        ref = Reference(prog, tla, cfg)
        _cache[name] = (prog, ref, ref.run())
    return _cache[name]


def level_lines_of_dump(path):
    """a dump file of state texts (`L<level> <state>` per line) -> the sorted state lines per level"""
    out = []
    for ln in open(path).read().splitlines():
        lv, _, text = ln.partition(" ")
        k = int(lv[1:])
        while len(out) < k:
            out.append([])
        out[k - 1].append(text)
    return [sorted(x) for x in out]


# ---- tests/_actshim: the host search that keeps the behaviour of the first violation, and -continue's rules with the invariant count
BINS, BIN_DEADLOCK, BIN_FATAL = 34, 32, 33   # violations.h


def build_actshim(csrc=None, out=None, own_front_end=False):
    """csrc: the directory the sources are taken from (default: the product's; a copy with one edit is a mutant).  own_front_end: the
    PlusCal front end of csrc is compiled INTO the library and bound to it (-Bsymbolic), whatever front end the process has loaded
    already; otherwise it is tests/_shim's library's"""
    import testlib
    src = helpers.ROOT / "tests" / "_actshim" / "actshim.cpp"
    csrc = csrc or testlib.CSRC
    if own_front_end:
        link = [csrc / f for f in testlib.FRONT_END]
        argv = ["-O0", *link, "-DACTSHIM_OWN_FRONT_END", "-Wl,-Bsymbolic"]
    else:
        link = [helpers.build_shim()]
        argv = ["-O1", "-L", link[0].parent, f"-l:{link[0].name}", f"-Wl,-rpath,{link[0].parent}"]
    return testlib.build_library((out or src.parent / "_build") / "libactshim.so",
                                 testlib.host_argv("-w", "-I", csrc, "-I", helpers.ROOT / "include", src, *argv), [src] + link + testlib.product_deps(csrc))


def actshim_lib(so=None):
    import ctypes as C

    class ActOut(C.Structure):
        _fields_ = [("distinct", C.c_uint64), ("generated", C.c_uint64), ("depth", C.c_uint32), ("trace_len", C.c_uint32), ("verdict", C.c_int32),
                    ("violated", C.c_int32), ("fatal", C.c_uint32), ("fatal_inv", C.c_uint32), ("fatal_pairs", C.c_uint64),
                    ("states", C.c_uint64 * BINS), ("outside", C.c_uint64 * BINS), ("levels", C.c_uint64 * 256)]
    L = C.CDLL(str(so or build_actshim()))
    L.ActOut = ActOut
    L.actshim_search.argtypes = [C.POINTER(C.c_int64), C.c_uint, C.c_int, C.POINTER(ActOut), C.c_char_p, C.c_char_p, C.c_size_t]
    L.actshim_pair.argtypes = [C.c_uint, C.c_int] + [C.POINTER(C.c_uint)] * 3
    L.actshim_stored_bin.argtypes = [C.c_uint, C.c_int]
    return L


def host_search(prog, cont=False, lib=None):
    """the interpreter's host build on a compiled program -> dict(verdict, violated (index), trace_len, distinct, generated, depth, levels,
    before / after (the last step of the first violation's behaviour, one line each), fatal, fatal_inv, fatal_pairs, states, outside)"""
    import ctypes as C
    L = lib or actshim_lib()
    o = L.ActOut()
    before, after = C.create_string_buffer(1 << 14), C.create_string_buffer(1 << 14)
    p = (C.c_int64 * len(prog.params))(*prog.params)
    assert L.actshim_search(p, len(prog.params), int(cont), C.byref(o), before, after, len(before)) == 0
    return dict(verdict=helpers.VERDICTS[o.verdict], violated=o.violated, trace_len=o.trace_len, distinct=o.distinct, generated=o.generated, depth=o.depth,
                levels=[o.levels[k] for k in range(o.depth)], before=before.value.decode().replace("\n", " "), after=after.value.decode().replace("\n", " "),
                fatal=bool(o.fatal), fatal_inv=o.fatal_inv, fatal_pairs=o.fatal_pairs, states=list(o.states), outside=list(o.outside))
