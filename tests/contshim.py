"""What -continue collects, on the host (tests/_contshim: tla_rust_amd/csrc/violations.h built with g++ over the spec lowerings, no
HIP), and what the references say it must be:

  * hand lowerings: the oracle's complete state graph (helpers.oracle_graph_files: the dump plus the edge file whose fifth column is the
    invariant a successor breaks);
  * compiled PlusCal: oracle/tla_eval.py's Checker — a plain BFS of the translation, every invariant evaluated on every state.

Both become a Reference: per entry (invariant index order, then deadlock, then the fatal error) the distinct stored states, the
successors outside the model, the level of the first one, and the whole-search counters as far as a search under -continue goes:
to the end of the level in which an Assert first fails, else the whole graph.

The library is built on first use, like tests/covshim.py's, and linked against helpers' libshim.so."""
import ctypes as C
import sys

import helpers

sys.path.insert(0, str(helpers.ROOT / "oracle"))

CONTSHIM_DIR = helpers.ROOT / "tests" / "_contshim"
SPECS = helpers.ROOT / "specs_continue"
BINS, BIN_DEADLOCK, BIN_FATAL = 34, 32, 33   # violations.h


class ContOut(C.Structure):
    _fields_ = [("states", C.c_uint64 * BINS), ("outside", C.c_uint64 * BINS), ("first_state", C.c_uint64 * BINS), ("first_level", C.c_uint32 * BINS),
                ("first_parent", C.c_uint64 * BINS), ("first_slot", C.c_uint32 * BINS), ("distinct", C.c_uint64), ("generated", C.c_uint64),
                ("depth", C.c_uint32), ("ninv", C.c_uint32), ("fatal", C.c_uint32), ("fatal_kind", C.c_uint32), ("levels", C.c_uint64 * 4096)]


def build_contshim(csrc=None, out=None):
    """csrc: the directory the lowerings and violations.h are taken from (default: the product's; a copy with one edit is a mutant)"""
    return helpers.build_over_shim((out or CONTSHIM_DIR / "_build") / "libcontshim.so", CONTSHIM_DIR / "contshim.cpp", csrc)


def load(so):
    L = C.CDLL(str(so))
    L.contshim_search.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_int, C.c_char_p, C.POINTER(ContOut)]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build_contshim())
    return _lib


def search(spec, params, deadlock=True, dump=None, L=None):
    """the host search under -continue: dict(entries=[dict(kind, invariant, states, outside, first_level, first_state)], distinct,
    generated, depth, levels); first_state: the dump's line of the first stored violator, or None"""
    L = L or lib()
    d = helpers.spec_desc(spec, params)
    o = ContOut()
    rc = L.contshim_search(C.byref(d), int(deadlock), str(dump).encode() if dump else None, C.byref(o))
    if rc:
        raise RuntimeError(f"contshim_search: {rc}")

    def entry(kind, inv, b):
        return dict(kind=kind, invariant=inv, states=o.states[b], outside=o.outside[b], first_level=o.first_level[b],
                    first_state=None if o.first_state[b] == 2 ** 64 - 1 else o.first_state[b])
    entries = [entry("invariant", k, k) for k in range(o.ninv)]
    if deadlock:
        entries.append(entry("deadlock", -1, BIN_DEADLOCK))
    if o.fatal:
        entries.append(entry({1: "invariant", 2: "assert", 4: "spec-error"}[o.fatal_kind], -1, BIN_FATAL))
    for b in range(o.ninv, 32):
        assert o.states[b] == 0 and o.outside[b] == 0, (b, "an invariant index the model does not have")
    return dict(entries=entries, distinct=o.distinct, generated=o.generated, depth=o.depth, levels=[o.levels[k] for k in range(o.depth)])


# ------------------------------------------------------------------------------------------------ the references
class Reference:
    """What a search under -continue must report.  Built from a complete graph:
    level[k], text[k] of stored state k; inv[k]: the first invariant state k breaks, or -1; dead[k]: no successor at all;
    edges: (parent index or -1, flags: 1 = a failed Assert / 2 = an evaluation error, in-model, invariant broken or -1, text)."""

    def __init__(self, names, level, text, inv, dead, edges, deadlock):
        self.names, self.level, self.text, self.inv, self.dead, self.edges, self.deadlock = names, level, text, inv, dead, edges, deadlock
        self.index = {t: k for k, t in enumerate(text)}
        # the search ends with the level whose expansion holds a fatal edge
        fatal = [(level[p], f) for p, f, _m, _i, _t in edges if p >= 0 and f & 3]
        self.fatal_level = min(lv for lv, _ in fatal) if fatal else None
        self.fatal_kind = None
        if fatal:
            kinds = {f & 3 for lv, f in fatal if lv == self.fatal_level}
            self.fatal_kind = "assert" if 1 in kinds else "spec-error"   # (the smallest key decides when a level holds both: not needed here)
        last = self.fatal_level + 1 if fatal else max(level)           # the deepest level that is stored
        self.expanded = self.fatal_level if fatal else max(level)      # ... and expanded
        self.kept = [k for k in range(len(level)) if level[k] <= last]
        self.depth = max(level[k] for k in self.kept)
        self.levels = [sum(1 for k in self.kept if level[k] == lv) for lv in range(1, self.depth + 1)]
        self.distinct = len(self.kept)
        self.generated = sum(1 for p, *_ in edges if p < 0 or level[p] <= self.expanded)
        self.succ = {}
        for p, f, m, i, t in edges:
            if p >= 0:
                self.succ.setdefault(text[p], set()).add(t)
        self.init_texts = {t for p, f, m, i, t in edges if p < 0}

    def entries(self):
        out = []
        for k, name in enumerate(self.names):
            st = [s for s in self.kept if self.inv[s] == k]
            outside = [(self.level[p], p) for p, f, m, i, t in self.edges if not f & 3 and not m and i == k and (p < 0 or self.level[p] <= self.expanded)]
            out.append(dict(kind="invariant", invariant=k, name=name, states=len(st), outside=len(outside),
                            first_level=min(self.level[s] for s in st) if st else (min(lv for lv, _ in outside) if outside else 0)))
        if self.deadlock:
            dl = [s for s in self.kept if self.dead[s] and self.level[s] <= self.expanded]
            out.append(dict(kind="deadlock", invariant=-1, name="Deadlock", states=len(dl), outside=0, first_level=min(self.level[s] for s in dl) if dl else 0))
        if self.fatal_level is not None:
            n = sum(1 for p, f, *_ in self.edges if p >= 0 and f & 3 and self.level[p] == self.fatal_level)
            out.append(dict(kind=self.fatal_kind, invariant=-1, name=self.fatal_kind, states=0, outside=n, first_level=self.fatal_level))
        return out

    def breaks(self, text, k):
        """does the stored state `text` break invariant k first?"""
        return self.inv[self.index[text]] == k

    def first_errors(self):
        """{(verdict, invariant index or -1, trace_len)}: everything the first flagged level holds — what a search WITHOUT the flag may
        report (it expands a level in parallel)"""
        errs = set()
        for k in range(len(self.level)):
            if self.inv[k] >= 0:
                errs.add((self.level[k] - 1 if self.level[k] > 1 else 0, "invariant", self.inv[k], self.level[k]))
            if self.dead[k] and self.deadlock:
                errs.add((self.level[k], "deadlock", -1, self.level[k]))
        for p, f, m, i, t in self.edges:
            if p >= 0 and f & 3:
                errs.add((self.level[p], "assert" if f & 1 else "spec-error", -1, self.level[p]))
            elif p >= 0 and not m and i >= 0:
                errs.add((self.level[p], "invariant", i, self.level[p] + 1))
        if not errs:
            return set()
        first = min(e[0] for e in errs)
        return {e[1:] for e in errs if e[0] == first}


def oracle_reference(spec, oparams, names, tmp, deadlock=True, check_on_expand=False):
    """the oracle's complete graph of a hand lowering.  check_on_expand: the lowering flags a state when it EXPANDS it (first_errors)"""
    dump, edges_path = tmp / "cont_states.txt", tmp / "cont_edges.txt"
    helpers.oracle_graph_files(spec, list(oparams), dump, edges_path, check_deadlock=deadlock)
    level, text = [], []
    with open(dump) as f:
        for line in f:
            lv, txt = line.rstrip("\n").split(" ", 1)
            level.append(int(lv[1:]))
            text.append(txt)
    index = {t: k for k, t in enumerate(text)}
    inv, dead, edges = [-1] * len(text), [True] * len(text), []
    with open(edges_path) as f:
        for line in f:
            par, _action, flags, inmodel, i, txt = line.rstrip("\n").split(" ", 5)
            par, flags, inmodel, i = int(par), int(flags), int(inmodel) == 1, int(i)
            edges.append((par, flags & 3, inmodel, i, txt))
            if par >= 0:
                dead[par] = False
            if not flags & 3 and inmodel:
                inv[index[txt]] = i
    ref = Reference(names, level, text, inv, dead, edges, deadlock)
    if check_on_expand:   # the state itself is the evidence, found one level later than a successor check finds it
        ref.first_errors = lambda: _first_errors_on_expand(ref)
    return ref


def _first_errors_on_expand(ref):
    errs = {(ref.level[k], "invariant", ref.inv[k], ref.level[k]) for k in range(len(ref.level)) if ref.inv[k] >= 0}
    errs |= {(ref.level[k], "deadlock", -1, ref.level[k]) for k in range(len(ref.level)) if ref.dead[k] and ref.deadlock}
    first = min(e[0] for e in errs) if errs else None
    return {e[1:] for e in errs if e[0] == first}


def checker_reference(translated, constants, invariants, constraints=(), deadlock=True):
    """oracle/tla_eval.py's Checker on a program's translation: a plain BFS, every invariant evaluated on every state"""
    from tla_eval import Checker
    ck = Checker(translated, constants=dict(constants or {}))
    ck.engine_mode = True   # (run_levels' convention: a failing Assert is one generated successor that is not stored)

    def line(s):
        return ck.fmt_state(s).replace("\n", " ")

    def first_broken(s):
        for k, name in enumerate(invariants):
            if not ck.ev(ck.defs[name][1], s, None, {}):
                return k
        return -1
    level, text, inv, dead, edges, states, seen = [], [], [], [], [], [], {}

    def store(s, lv):
        seen[ck.key(s)] = len(text)
        level.append(lv)
        text.append(line(s))
        inv.append(first_broken(s))
        dead.append(True)
        states.append(s)
    for s in ck.initial_states():
        m = ck.in_model(s, constraints)
        edges.append((-1, 0, m, first_broken(s), line(s)))
        if m and ck.key(s) not in seen:
            store(s, 1)
    k = 0
    while k < len(states):
        for n in ck.successors(states[k]):
            dead[k] = False
            if "__assert__" in n:
                edges.append((k, 1, False, -1, "-"))
                continue
            m = ck.in_model(n, constraints)
            edges.append((k, 0, m, first_broken(n), line(n)))
            if m and ck.key(n) not in seen:
                store(n, level[k] + 1)
        k += 1
    return Reference(list(invariants), level, text, inv, dead, edges, deadlock)


def module(name):
    """(text, invariants, constants, constraints, deadlock) of specs_continue/<name>: the cfg's statements, read the simple way"""
    text = (SPECS / f"{name}.tla").read_text()
    cfg = (SPECS / f"{name}.cfg").read_text()
    invs, cons, consts, deadlock = [], [], {}, True
    for ln in cfg.splitlines():
        w = ln.split()
        if not w:
            continue
        if w[0] in ("INVARIANT", "INVARIANTS"):
            invs += w[1:]
        elif w[0] in ("CONSTRAINT", "CONSTRAINTS"):
            cons += w[1:]
        elif w[0] in ("CONSTANT", "CONSTANTS"):
            for k in range(1, len(w), 3):
                consts[w[k]] = int(w[k + 2])
        elif w[0] == "CHECK_DEADLOCK":
            deadlock = w[1] == "TRUE"
    return text, invs, consts, cons, deadlock
