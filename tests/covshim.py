"""Host counts of -coverage (tests/_covshim: tla_rust_amd/csrc/coverage.h built with g++ over the spec lowerings, no HIP), and what the
oracle's state graph says the counts must be.

The library is built on first use, like tests/simwalk.py's, and linked against helpers' libshim.so."""
import ctypes as C
from collections import Counter

import helpers

COVSHIM_DIR = helpers.ROOT / "tests" / "_covshim"
MAX_BINS = 512   # coverage.h COV_MAX_BINS


def build_covshim(csrc=None, out=None):
    """csrc: the directory the lowerings and coverage.h are taken from (default: the product's; a copy with one edit is a mutant)"""
    return helpers.build_over_shim((out or COVSHIM_DIR / "_build") / "libcovshim.so", COVSHIM_DIR / "covshim.cpp", csrc)


def load(so):
    L = C.CDLL(str(so))
    L.covshim_search.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int),
                                 C.POINTER(C.c_uint64)]
    L.covshim_listed.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_int]
    L.covshim_action_name.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_int]
    L.covshim_action_name.restype = C.c_char_p
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build_covshim())
    return _lib


def search(spec, params, dump=None, L=None):
    """the host search of the whole graph: dict(generated={name: n}, distinct={name: n}, states=n); names: "Init" and every action of
    the model, zero rows included"""
    L = L or lib()
    d = helpers.spec_desc(spec, params)
    gen, dis = (C.c_uint64 * MAX_BINS)(), (C.c_uint64 * MAX_BINS)()
    nb, ns = C.c_int(0), C.c_uint64(0)
    rc = L.covshim_search(C.byref(d), str(dump).encode() if dump else None, gen, dis, C.byref(nb), C.byref(ns))
    if rc:
        raise RuntimeError(f"covshim_search: {rc}")
    out = dict(generated={"Init": gen[0]}, distinct={"Init": dis[0]}, states=ns.value)
    for a in range(nb.value - 1):
        if L.covshim_listed(C.byref(d), a):
            name = L.covshim_action_name(C.byref(d), a).decode()
            assert name not in out["generated"], name
            out["generated"][name], out["distinct"][name] = gen[a + 1], dis[a + 1]
        else:
            assert gen[a + 1] == 0 and dis[a + 1] == 0, (a, gen[a + 1], dis[a + 1])   # an id that is no action of the model never counts
    return out


# ------------------------------------------------------------------------------------------------ the oracle's graph
class OracleGraph:
    """the oracle's complete state graph (helpers.oracle_graph_files): level[k] of stored state k, text[k], and the edges as
    (parent index or -1, action name, flags, in-model, text)"""

    def __init__(self, spec, oparams, tmp, check_deadlock=True):
        dump, edges = tmp / "cov_states.txt", tmp / "cov_edges.txt"
        self.counters = helpers.oracle_graph_files(spec, list(oparams), dump, edges, check_deadlock=check_deadlock)
        name = helpers.oracle_lib().oracle_action_name
        self.level, self.text = [], []
        with open(dump) as f:
            for line in f:
                lv, txt = line.rstrip("\n").split(" ", 1)
                self.level.append(int(lv[1:]))
                self.text.append(txt)
        self.index = {t: k for k, t in enumerate(self.text)}
        assert len(self.index) == len(self.text)
        self.edges = []
        names = {}
        with open(edges) as f:
            for line in f:
                par, action, flags, inmodel, _inv, text = line.rstrip("\n").split(" ", 5)
                a = int(action)
                if a not in names:
                    names[a] = name(spec.encode(), a).decode()
                self.edges.append((int(par), names[a] if int(par) >= 0 else "Init", int(flags), int(inmodel) == 1, text))
        self.depth = max(self.level)

    def generated(self, expanded_levels=None):
        """{action name: edges out of parents of levels 1 .. expanded_levels} (None: every level) + "Init": the initial states generated"""
        c = Counter()
        for par, name, _f, _m, _t in self.edges:
            if par < 0 or expanded_levels is None or self.level[par] <= expanded_levels:
                c[name] += 1
        return c

    def distinct_bounds(self, expanded_levels=None):
        """({name: lower}, {name: upper}, stored) for the states a search that expanded levels 1 .. expanded_levels stores: a state of
        level L was first found by one of the edges that lead to it from level L - 1 (initial states: by Init) — which one is the
        search's race.  upper[a]: states with such an edge of action a; lower[a]: states ALL of whose such edges are of action a."""
        cand = {}
        for par, name, flags, inmodel, text in self.edges:
            if flags & 3 or not inmodel:   # a failed Assert / an evaluation error has no state; an out-of-model successor is not stored
                continue
            k = self.index[text]
            if (par < 0 and self.level[k] == 1) or (par >= 0 and self.level[par] + 1 == self.level[k]):
                cand.setdefault(k, set()).add(name)
        lower, upper, stored = Counter(), Counter(), 0
        for k, lv in enumerate(self.level):
            if expanded_levels is not None and lv > expanded_levels + 1:
                continue
            stored += 1
            names = cand[k]
            for nm in names:
                upper[nm] += 1
            if len(names) == 1:
                lower[next(iter(names))] += 1
        return lower, upper, stored
