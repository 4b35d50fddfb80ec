"""Host build of the checks label by label (tests/_unitshim: the front end's unit map, liveness.h's live_edge_unit and the rule over
units built with g++ over the interpreter lowering, no HIP; pcal.cpp / pcal_compile.cpp are compiled in, so that a copy of csrc with one
edit is a mutant of the front end too).  Built on first use."""
import ctypes as C

import helpers
import testlib

SHIM_DIR = helpers.ROOT / "tests" / "_unitshim"


class FairUnits(C.Structure):
    """mc_fair_units"""
    _fields_ = [("nunits", C.c_int32), ("nconj", C.c_int32), ("of_unit", C.c_uint64 * 128), ("weak_mask", C.c_uint64), ("strong_mask", C.c_uint64)]


def build(csrc=None, out=None, shim_src=None):
    """csrc: the directory the front end, the lowerings and liveness.h are taken from (default: the product's; a copy with one edit is
    a mutant); shim_src: unitshim.cpp or an edited copy"""
    csrc = csrc or testlib.CSRC
    shim_src = shim_src or SHIM_DIR / "unitshim.cpp"
    front = [csrc / f for f in testlib.FRONT_END]
    return testlib.build_library((out or SHIM_DIR / "_build") / "libunitshim.so", testlib.host_argv("-O1", "-Wl,-Bsymbolic", "-I", csrc, shim_src, *front),
                                 [shim_src] + front + testlib.product_deps(csrc))


def load(so):
    L = C.CDLL(str(so))
    L.unitshim_compile.restype = C.c_void_p
    L.unitshim_compile.argtypes = [C.c_char_p, C.c_char_p]
    L.unitshim_error.restype = C.c_char_p
    L.unitshim_free.argtypes = [C.c_void_p]
    L.unitshim_table.argtypes = [C.c_void_p, C.POINTER(FairUnits), C.c_char_p, C.c_size_t]
    L.unitshim_check.argtypes = [C.POINTER(helpers.McSpecDesc), C.POINTER(FairUnits), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p,
                                 C.POINTER(C.c_uint64)]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build())
    return _lib


class Program:
    """a module compiled by THIS library's front end: the table of units and conjuncts, and the checks"""

    def __init__(self, tla_text, cfg_text, L=None):
        self.L = L or lib()
        props = [w for line in cfg_text.splitlines() if line.startswith(("PROPERTY", "PROPERTIES")) for w in line.split()[1:] if w != "Termination"]
        self.h = self.L.unitshim_compile(tla_text.encode(), ",".join(props).encode())
        if not self.h:
            raise RuntimeError(self.L.unitshim_error().decode())
        self.fu = FairUnits()
        buf = C.create_string_buffer(1 << 16)
        n = self.L.unitshim_table(self.h, C.byref(self.fu), buf, len(buf))
        self.refusal = self.L.unitshim_error().decode() if n < 0 else None
        self.conjuncts = buf.value.decode().splitlines()

    def close(self):
        if self.h:
            self.L.unitshim_free(self.h)
            self.h = None

    def check(self, prop, tmp):
        """one check (prop["kind"] < 0: Termination): a dict with texts (the states in the shim's order), violated, final (the final
        components as a set of frozensets of state texts), rounds, closed, and edges = [(source text, successor text, unit, the set of
        the unit's conjuncts)]"""
        d = helpers.spec_desc("pcal", [self.h])
        states, out, edges = (tmp / f"unit_{k}.txt" for k in ("states", "out", "edges"))
        counts = (C.c_uint64 * 8)()
        rc = self.L.unitshim_check(C.byref(d), C.byref(self.fu), prop["kind"], prop["p"], prop["q"], str(states).encode(), str(out).encode(),
                                   str(edges).encode(), counts)
        if rc:
            raise RuntimeError(f"unitshim_check: {rc}")
        texts = [line.rstrip("\n") for line in open(states)]
        comps = {}
        for t, line in zip(texts, open(out)):
            i, st = map(int, line.split())
            if st == 2:
                comps.setdefault(i, set()).add(t)
        es = []
        for line in open(edges):
            i, j, u, mask = line.split()
            es.append((texts[int(i)], texts[int(j)], int(u), {k for k in range(64) if int(mask, 16) >> k & 1}))
        return dict(texts=texts, violated=bool(counts[5]), final={frozenset(m) for m in comps.values()}, rounds=counts[3], closed=counts[6],
                    overrun=counts[7], edges=es)
