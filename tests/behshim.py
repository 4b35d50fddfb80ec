"""The behaviour rule on the host (tests/_behshim: tla_rust_amd/csrc/behaviour.h built with g++ over the spec lowerings, no HIP).

Built on first use, like simwalk's library, and linked against helpers' libshim.so for the PlusCal front-end.  Rows are bytes
(8 * words each), as the Python binding hands them around."""
import ctypes as C

import helpers
import testlib

BEHSHIM_DIR = helpers.ROOT / "tests" / "_behshim"
VERDICTS = {1: "accepted", 2: "rejected", 3: "ambiguous"}
FIELDS = ("verdict", "step", "candidates", "peak", "generated", "outside", "errors")
ST_ENABLED, ST_OUT_OF_MODEL, ST_ASSERT, ST_INVARIANT, ST_SPECERR, ST_OVERFLOW, ST_SELFLOOP = 1, 2, 4, 8, 16, 32, 64
STUTTER = 1


class Verdict(C.Structure):
    _fields_ = [("verdict", C.c_int32), ("step", C.c_uint32), ("candidates", C.c_uint32), ("peak", C.c_uint32),
                ("generated", C.c_uint64), ("outside", C.c_uint64), ("errors", C.c_uint64)]

    def as_dict(self):
        return dict(verdict=VERDICTS[self.verdict], **{f: getattr(self, f) for f in FIELDS[1:]})


def build(csrc=None, out=None):
    """the host library; csrc: where the lowerings and behaviour.h come from (default: the product's; a copy with one line edited is
    how the mutants are built), out: where the library goes"""
    return helpers.build_over_shim((out or BEHSHIM_DIR / "_build") / "libbehshim.so", BEHSHIM_DIR / "behshim.cpp", csrc)


def load(so):
    L = C.CDLL(str(so))
    D = C.POINTER(helpers.McSpecDesc)
    L.behshim_words.argtypes = [D]
    L.behshim_format.argtypes = [D, C.c_char_p, C.c_char_p, C.c_size_t]
    L.behshim_check.argtypes = [D, C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p, C.c_char_p, C.c_uint, C.POINTER(Verdict)]
    L.behshim_sets.argtypes = [D, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint, C.POINTER(Verdict), C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t,
                               C.c_char_p, C.POINTER(C.c_int32)]
    L.behshim_sets.restype = C.c_long
    L.behshim_init.argtypes = [D, C.c_uint64, C.c_char_p]
    L.behshim_init.restype = C.c_long
    L.behshim_succ.argtypes = [D, C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_int)]
    L.behshim_succ.restype = C.c_uint
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build())
    return _lib


class Model:
    """a lowering seen through the shim: rows, texts, the rule"""

    def __init__(self, spec, params, L=None):
        self.spec, self.params, self.L = spec, list(params), L or lib()
        self.d = helpers.spec_desc(spec, params)
        self.W = 8 * self.L.behshim_words(C.byref(self.d))

    def fmt(self, row):
        buf = C.create_string_buffer(1 << 16)
        n = self.L.behshim_format(C.byref(self.d), row, buf, len(buf))
        return buf.raw[:n].decode().replace("\n", " ")

    def inits(self):
        buf = C.create_string_buffer(self.W)
        n = self.L.behshim_init(C.byref(self.d), 1 << 62, buf)
        out = []
        for k in range(n):
            self.L.behshim_init(C.byref(self.d), k, buf)
            out.append(buf.raw)
        return out

    def successors(self, row):
        """[(slot, status, successor row or None for an error)] of the enabled slots"""
        out, ns, buf = [], C.c_int(0), C.create_string_buffer(self.W)
        self.L.behshim_succ(C.byref(self.d), row, -1, buf, C.byref(ns))
        for slot in range(ns.value):
            st = self.L.behshim_succ(C.byref(self.d), row, slot, buf, C.byref(ns))
            if st & ST_ENABLED:
                out.append((slot, st, None if st & (ST_ASSERT | ST_SPECERR | ST_OVERFLOW) else buf.raw))
        return out

    def reachable(self, limit=200000):
        """{text: row} of the states reachable through in-model steps, and {row: [(slot, status, successor)]} of those expanded"""
        by_text, succ, todo = {}, {}, []
        for r in self.inits():
            by_text.setdefault(self.fmt(r), r)
            todo.append(r)
        while todo:
            r = todo.pop()
            if r in succ:
                continue
            succ[r] = self.successors(r)
            assert len(succ) <= limit
            for _, st, t in succ[r]:
                if t is not None:
                    by_text.setdefault(self.fmt(t), t)
                    if not st & ST_OUT_OF_MODEL and t not in succ:
                        todo.append(t)
        return by_text, succ

    def _batch(self, rows_list, mask):
        first = (C.c_uint64 * (len(rows_list) + 1))()
        for b, rows in enumerate(rows_list):
            assert all(len(r) == self.W for r in rows)
            first[b + 1] = first[b] + len(rows)
        assert mask is None or len(mask) == self.W
        return first, b"".join(b"".join(rows) for rows in rows_list)

    def check(self, rows_list, mask=None, stutter=False):
        """the verdicts of a batch, as dicts with the fields of mc_beh_verdict"""
        first, blob = self._batch(rows_list, mask)
        out = (Verdict * max(len(rows_list), 1))()
        rc = self.L.behshim_check(C.byref(self.d), len(rows_list), first, blob, mask, STUTTER if stutter else 0, out)
        assert rc == 0, rc
        return [v.as_dict() for v in out[:len(rows_list)]]

    def sets(self, rows, mask=None, stutter=False):
        """(verdict, [K_0, K_1, ...] as lists of rows, witness [(slot, row)]) of one behaviour"""
        v, sizes = Verdict(), (C.c_uint32 * len(rows))()
        cap = 64 * len(rows)
        buf, wr, ws = C.create_string_buffer(cap * self.W), C.create_string_buffer(len(rows) * self.W), (C.c_int32 * len(rows))()
        n = self.L.behshim_sets(C.byref(self.d), b"".join(rows), len(rows), mask, STUTTER if stutter else 0, C.byref(v), sizes, buf, cap, wr, ws)
        assert n >= 0
        out, at = [], 0
        for i in range(n):
            out.append([buf.raw[(at + k) * self.W:(at + k + 1) * self.W] for k in range(sizes[i])])
            at += sizes[i]
        return v.as_dict(), out, [(ws[k], wr.raw[k * self.W:(k + 1) * self.W]) for k in range(n)]


# ------------------------------------------------------------------------------------------------ the kernel over a test lowering
def build_device(mutant=0):
    """tests/_behshim/behshim.hip: k_behaviours over the lowering SpecHide, a library of its own (hipcc cross-compiles gfx950 without a
    GPU); mutant 1 / 2 / 3: the kernel with one thing broken"""
    src = BEHSHIM_DIR / "behshim.hip"
    return testlib.build_library(BEHSHIM_DIR / "_build" / f"libbehdev{mutant}.so",
                                 testlib.hip_argv(f"-DBEH_MUTANT={mutant}", "-I", helpers.ROOT / "include", "-I", testlib.CSRC, src),
                                 [src] + testlib.product_deps(testlib.CSRC))


def build_devices():
    return list(testlib.build_mutants(range(4), build_device).values())


class HideModel:
    """SpecHide of behshim.hip: rows are (x, h) pairs; host(): the host rule, device(): this library's kernel"""

    def __init__(self, mutant=0):
        self.L = C.CDLL(str(build_device(mutant)))
        args = [C.c_uint64, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint]
        self.L.bd_host.argtypes = args + [C.POINTER(Verdict)]
        self.L.bd_device.argtypes = args + [C.c_uint32, C.POINTER(Verdict)]
        self.L.bd_last_error.restype = C.c_char_p
        assert self.L.bd_mutant() == mutant

    def _args(self, K, B, batch, mask, stutter):
        first = (C.c_uint64 * (len(batch) + 1))()
        flat = []
        for b, rows in enumerate(batch):
            first[b + 1] = first[b] + len(rows)
            flat += [w for r in rows for w in r]
        m = (C.c_uint64 * 2)(*mask) if mask is not None else None
        return [K, B, len(batch), first, (C.c_uint64 * len(flat))(*flat), m, STUTTER if stutter else 0], (Verdict * len(batch))()

    def host(self, K, B, batch, mask=None, stutter=False):
        a, out = self._args(K, B, batch, mask, stutter)
        assert self.L.bd_host(*a, out) == 0
        return [v.as_dict() for v in out]

    def device(self, K, B, batch, mask=None, stutter=False, iters=3):
        a, out = self._args(K, B, batch, mask, stutter)
        rc = self.L.bd_device(*a, iters, out)
        assert rc == 0, (rc, self.L.bd_last_error())
        return [v.as_dict() for v in out]
