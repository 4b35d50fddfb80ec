"""Host build of the state graph (tests/_graphshim: tla_rust_amd/csrc/graph.h built with g++ over the spec lowerings, no HIP), and the
edge multiset the oracle's state graph says it must be.

The library is built on first use, like tests/covshim.py's, and linked against helpers' libshim.so."""
import ctypes as C
from collections import Counter

import helpers

GRAPHSHIM_DIR = helpers.ROOT / "tests" / "_graphshim"


def build_graphshim(csrc=None, out=None):
    """csrc: the directory the lowerings and graph.h are taken from (default: the product's; a copy with one edit is a mutant)"""
    return helpers.build_over_shim((out or GRAPHSHIM_DIR / "_build") / "libgraphshim.so", GRAPHSHIM_DIR / "graphshim.cpp", csrc)


def load(so):
    L = C.CDLL(str(so))
    L.graphshim_search.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_uint64, C.c_int, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64)]
    L.graphshim_action_name.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_int]
    L.graphshim_action_name.restype = C.c_char_p
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build_graphshim())
    return _lib


COUNTS = ("states", "edges", "self_loops", "dropped", "missing", "left_home", "generated")


def search(spec, params, nbuckets, sparse, tmp, L=None):
    """the host search over a seen-set of `nbuckets` buckets (sparse: MC_SPARSE_SLOTS slots each, else 8), then graph.h over every state:
    (counts dict, texts [state k], Counter of (source text, action name, destination text))"""
    L = L or lib()
    d = helpers.spec_desc(spec, params)
    states, edges = tmp / "host_graph_states.txt", tmp / "host_graph_edges.txt"
    counts = (C.c_uint64 * 7)()
    rc = L.graphshim_search(C.byref(d), nbuckets, 1 if sparse else 0, str(states).encode(), str(edges).encode(), counts)
    if rc:
        raise RuntimeError(f"graphshim_search: {rc}")
    texts = [line.rstrip("\n").split(" ", 1)[1] for line in open(states)]
    names, multiset = {}, Counter()
    for line in open(edges):
        src, a, dst = map(int, line.split())
        if a not in names:
            names[a] = L.graphshim_action_name(C.byref(d), a).decode()
        multiset[(texts[src], names[a], texts[dst])] += 1
    return dict(zip(COUNTS, counts)), texts, multiset


def oracle_edges(g, expanded_levels=None):
    """the reference multiset of a covshim.OracleGraph: (parent text, action name, successor text) over the edges whose parent lies in
    an expanded level (None: every level), that carry no Assert / evaluation-error flag, and whose successor is in-model and stored
    within the levels kept (levels 1 .. expanded_levels + 1)"""
    out = Counter()
    for par, name, flags, inmodel, text in g.edges:
        if par < 0 or flags & 3 or not inmodel:
            continue
        if expanded_levels is not None and g.level[par] > expanded_levels:
            continue
        k = g.index.get(text)
        if k is None or (expanded_levels is not None and g.level[k] > expanded_levels + 1):
            continue
        out[(g.text[par], name, text)] += 1
    return out


def engine_edges(eng, info, offsets, dst, act):
    """the engine's multiset from Engine.graph() + state_texts + mc_action_name; also the texts, one line each"""
    import numpy as np
    import tla_rust_amd.binding as b
    texts = [t.replace("\n", " ") for t in eng.state_texts(0, info.states)]
    src = np.repeat(np.arange(info.states, dtype=np.int64), np.diff(offsets.astype(np.int64)))
    names = {}
    out = Counter()
    for (i, a, j), n in Counter(zip(src.tolist(), act.tolist(), dst.tolist())).items():   # (equal rows are translated once)
        if a not in names:
            names[a] = b.lib().mc_action_name(C.byref(eng.desc), a).decode()
        out[(texts[i], names[a], texts[j])] += n
    return out, texts
