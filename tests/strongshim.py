"""Host build of the rule for liveness under strong process fairness (tests/_strongshim: tla_rust_amd/csrc/liveness.h built with g++
over the compiled-program lowering, no HIP).  Built on first use, like tests/livepropshim.py's library, and linked against helpers'
libshim.so."""
import ctypes as C

import helpers

SHIM_DIR = helpers.ROOT / "tests" / "_strongshim"


def build(csrc=None, out=None):
    """csrc: the directory the lowerings and liveness.h are taken from (default: the product's; a copy with one edit is a mutant)"""
    return helpers.build_over_shim((out or SHIM_DIR / "_build") / "libstrongshim.so", SHIM_DIR / "strongshim.cpp", csrc)


def load(so):
    L = C.CDLL(str(so))
    L.strongshim_check.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                   C.POINTER(C.c_uint64)]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build())
    return _lib


def check(program, weak, strong, prop, tmp, L=None):
    """liveness.h's refinement over the program's whole state graph for one check (prop["kind"] < 0: Termination): a dict with texts
    (the states in the shim's order), final (the final components as a set of frozensets of state texts), ids (text -> the text of the
    state whose index is the refined id), dist, witness (text or None; Termination: the least final root's) and the counts"""
    L = L or lib()
    d = helpers.spec_desc("pcal", program.params)
    states, out = tmp / "strong_states.txt", tmp / "strong_out.txt"
    counts = (C.c_uint64 * 8)()
    rc = L.strongshim_check(C.byref(d), weak, strong, prop["kind"], prop["p"], prop["q"], str(states).encode(), str(out).encode(), counts)
    if rc:
        raise RuntimeError(f"strongshim_check: {rc}")
    texts = [line.rstrip("\n") for line in open(states)]
    comps, ids, dist = {}, {}, {}
    for t, line in zip(texts, open(out)):
        i, st, dd = map(int, line.split())
        ids[t] = texts[i]
        dist[t] = None if dd < 0 else dd
        if st == 2:
            comps.setdefault(i, set()).add(t)
    witness = None if counts[2] == 2 ** 64 - 1 else texts[counts[2]]
    return dict(texts=texts, final={frozenset(m) for m in comps.values()}, ids=ids, dist=dist, witness=witness, states=counts[0],
                components=counts[1], rounds=counts[3], mask_states=counts[4], bad_starts=counts[5], closed=counts[6], overrun=counts[7])
