"""Host build of the Termination rule (tests/_liveshim: tla_rust_amd/csrc/liveness.h built with g++ over the compiled-program lowering,
no HIP).  Built on first use, like tests/graphshim.py's library, and linked against helpers' libshim.so."""
import ctypes as C

import helpers

LIVESHIM_DIR = helpers.ROOT / "tests" / "_liveshim"


def build_liveshim(csrc=None, out=None):
    """csrc: the directory the lowerings and liveness.h are taken from (default: the product's; a copy with one edit is a mutant)"""
    return helpers.build_over_shim((out or LIVESHIM_DIR / "_build") / "libliveshim.so", LIVESHIM_DIR / "liveshim.cpp", csrc)


def load(so):
    L = C.CDLL(str(so))
    L.liveshim_check.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_uint64, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64)]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build_liveshim())
    return _lib


def check(program, fair_mask, tmp, L=None):
    """liveness.h over the program's whole state graph: (partition: set of frozensets of state texts, the fair non-Done components among
    them as a set, counts dict)"""
    L = L or lib()
    d = helpers.spec_desc("pcal", program.params)
    states, out = tmp / "live_states.txt", tmp / "live_out.txt"
    counts = (C.c_uint64 * 4)()
    rc = L.liveshim_check(C.byref(d), fair_mask, str(states).encode(), str(out).encode(), counts)
    if rc:
        raise RuntimeError(f"liveshim_check: {rc}")
    texts = [line.rstrip("\n") for line in open(states)]
    comps, bad = {}, set()
    for t, line in zip(texts, open(out)):
        c, b = map(int, line.split())
        comps.setdefault(c, set()).add(t)
        if b:
            bad.add(c)
    return {frozenset(m) for m in comps.values()}, {frozenset(comps[c]) for c in bad}, dict(zip(("states", "components", "violating", "procs"), counts))
