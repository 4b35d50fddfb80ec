"""Host build of the rule for <>Q, []<>Q, <>[]P and P ~> Q (tests/_livepropshim: tla_rust_amd/csrc/liveness.h built with g++ over the
compiled-program lowering, no HIP).  Built on first use, like tests/liveshim.py's library, and linked against helpers' libshim.so."""
import ctypes as C

import helpers

SHIM_DIR = helpers.ROOT / "tests" / "_livepropshim"


def build(csrc=None, out=None):
    """csrc: the directory the lowerings and liveness.h are taken from (default: the product's; a copy with one edit is a mutant)"""
    return helpers.build_over_shim((out or SHIM_DIR / "_build") / "liblivepropshim.so", SHIM_DIR / "livepropshim.cpp", csrc)


def load(so):
    L = C.CDLL(str(so))
    L.livepropshim_check.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64)]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build())
    return _lib


def check(program, fair_mask, prop, tmp, L=None):
    """liveness.h over the program's whole state graph for one entry of Program.live_properties: a dict with texts (the states in the
    shim's order), bits, violating (the violating components as a set of frozensets of state texts), bad (the texts of their states),
    dist (text -> distance or None), witness (text or None) and the counts states / components / preds / mask_states / bad_starts"""
    L = L or lib()
    d = helpers.spec_desc("pcal", program.params)
    states, out = tmp / "prop_states.txt", tmp / "prop_out.txt"
    counts = (C.c_uint64 * 6)()
    rc = L.livepropshim_check(C.byref(d), fair_mask, prop["kind"], prop["p"], prop["q"], str(states).encode(), str(out).encode(), counts)
    if rc:
        raise RuntimeError(f"livepropshim_check: {rc}")
    texts = [line.rstrip("\n") for line in open(states)]
    bits, comps, bad, dist = [], {}, set(), {}
    for t, line in zip(texts, open(out)):
        b, c, v, dd = map(int, line.split())
        bits.append(b)
        comps.setdefault(c, set()).add(t)
        dist[t] = None if dd < 0 else dd
        if v:
            bad.add(t)
    violating = {frozenset(m & bad) for m in comps.values() if m & bad}
    witness = None if counts[2] == 2 ** 64 - 1 else texts[counts[2]]
    return dict(texts=texts, bits=bits, violating=violating, bad=bad, dist=dist, witness=witness, states=counts[0], components=counts[1],
                preds=counts[3], mask_states=counts[4], bad_starts=counts[5])
