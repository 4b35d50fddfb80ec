"""A test-only driver of the product's StateGraph (tests/_sgraph/sgraph.hip compiled together with tla_rust_amd/csrc/state_graph.hip
into a library of its own, without libtlamc.so): the strongly-connected-components pass, the fairness checks, the counterexample builder
and the two device scans on CSR arrays that no search of a model produced (tests/randgraph.py).  Built on first use, like
tests/livepropshim.py's library; hipcc cross-compiles gfx950 without a GPU, loading the library needs none either."""
import ctypes as C

import numpy as np

import helpers
import testlib

SHIM_DIR = helpers.ROOT / "tests" / "_sgraph"
CSRC = helpers.ROOT / "tla_rust_amd" / "csrc"
SCC_BATCH = 8   # engine_live.h: sweeps between two reads of the "changed" flag


class SccInfo(C.Structure):
    """mc_scc_info (as tla_rust_amd/binding.py has it)"""
    _fields_ = [("states", C.c_uint64), ("components", C.c_uint64), ("nontrivial", C.c_uint64), ("largest", C.c_uint64),
                ("trim_rounds", C.c_uint32), ("colour_rounds", C.c_uint32), ("backward_rounds", C.c_uint32), ("passes", C.c_uint32),
                ("seconds", C.c_double)]


class LiveInfo(C.Structure):
    """mc_live_info"""
    _fields_ = [("violated", C.c_int32), ("pad", C.c_uint32), ("fair_components", C.c_uint64), ("root", C.c_uint64),
                ("root_size", C.c_uint64), ("seconds", C.c_double)]


class LiveCheckInfo(C.Structure):
    """mc_live_check_info"""
    _fields_ = [("violated", C.c_int32), ("sweeps", C.c_uint32), ("fair_components", C.c_uint64), ("witness", C.c_uint64), ("root", C.c_uint64),
                ("root_size", C.c_uint64), ("mask_states", C.c_uint64), ("bad_starts", C.c_uint64), ("scc_builds", C.c_uint32), ("pad", C.c_uint32),
                ("seconds", C.c_double)]


def build(csrc=None, out=None):
    """csrc: the directory state_graph.hip, engine_live.h and the headers they include are taken from (default: the product's; a copy
    with one edit is a mutant); out: where the library goes"""
    return build_driver((out or SHIM_DIR / "_build") / "libsgraph.so", csrc or CSRC, [SHIM_DIR / "sgraph.hip"])


def build_driver(so, csrc, drivers):
    """drivers[0] (which includes the rest of `drivers` whole) compiled together with csrc's state_graph.hip: sfgraph's and ufgraph's too"""
    include = csrc.parent.parent / "include"   # (state_graph.h includes ../../include/tlamc.h: a copy of csrc brings its own)
    return testlib.build_library(so, testlib.hip_argv("-I", include, "-I", csrc, drivers[0], csrc / "state_graph.hip"),
                                 drivers + [csrc / "state_graph.hip"] + testlib.product_deps(csrc))


def load(so):
    L = C.CDLL(str(so))
    u64, u32p, vp = C.c_uint64, C.POINTER(C.c_uint32), C.c_void_p
    L.sg_last_error.restype = C.c_char_p
    L.sg_create.restype = vp
    L.sg_create.argtypes = [u64, u64, u64, C.POINTER(C.c_uint64), u32p, C.POINTER(C.c_int8), u32p]
    L.sg_destroy.argtypes = [vp]
    L.sg_destroy.restype = None
    L.sg_scc.argtypes = [vp, C.POINTER(SccInfo)]
    for f in (L.sg_scc_read, L.sg_live_scc_read, L.sg_pred_read):
        f.argtypes = [vp, u64, u64, u32p]
    L.sg_live_check.argtypes = [vp, u64, u64, C.POINTER(LiveInfo)]
    L.sg_live_check_masked.argtypes = [vp, u64, u64, C.c_int, C.c_int, C.c_int, C.POINTER(LiveCheckInfo)]
    L.sg_live_trace.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t, u32p, C.POINTER(C.c_size_t), u32p, C.POINTER(C.c_size_t)]
    L.sg_scan_exclusive_u32_to_u64.argtypes = [u32p, C.POINTER(C.c_uint64), u64]
    L.sg_scan_answers_inclusive.argtypes = [C.POINTER(C.c_uint8), u32p, u64]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build())
    return _lib


class SgError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} (code {code})")
        self.code = code


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _fields(s):
    return {k: getattr(s, k) for k, _ in s._fields_ if k != "pad"}


class Graph:
    """one mc::StateGraph over the given arrays.  proc (per edge, -1 = the terminating disjunct) and pred (per state) are optional: the
    fairness checks need the first, the property checks both."""

    def __init__(self, offsets, dst, proc=None, pred=None, ninit=0, L=None):
        self.L = L or lib()
        self.n, self.edges = len(offsets) - 1, len(dst)
        self._keep = [np.ascontiguousarray(offsets, dtype=np.uint64), np.ascontiguousarray(dst, dtype=np.uint32),
                      None if proc is None else np.ascontiguousarray(proc, dtype=np.int8),
                      None if pred is None else np.ascontiguousarray(pred, dtype=np.uint32)]
        o, d, pr, pd = self._keep
        assert pr is None or len(pr) == self.edges
        assert pd is None or len(pd) == self.n
        self.h = self.L.sg_create(self.n, self.edges, ninit, _ptr(o, C.c_uint64), _ptr(d, C.c_uint32),
                                  None if pr is None else _ptr(pr, C.c_int8), None if pd is None else _ptr(pd, C.c_uint32))
        if not self.h:
            raise SgError(-1, self.L.sg_last_error().decode())

    def close(self):
        if self.h:
            self.L.sg_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ok(self, rc):
        if rc:
            raise SgError(rc, self.L.sg_last_error().decode())

    def _read(self, f, first, count):
        out = np.empty(count, dtype=np.uint32)
        self._ok(f(self.h, first, count, _ptr(out, C.c_uint32)))
        return out

    def scc(self):
        """(the mc_scc_info's fields, the component ids of all states)"""
        si = SccInfo()
        self._ok(self.L.sg_scc(self.h, C.byref(si)))
        return _fields(si), self.scc_read(0, self.n)

    def scc_read(self, first, count):
        return self._read(self.L.sg_scc_read, first, count)

    def live_scc_read(self, first, count):
        return self._read(self.L.sg_live_scc_read, first, count)

    def pred_read(self, first, count):
        return self._read(self.L.sg_pred_read, first, count)

    def live_check(self, all_mask, fair):
        li = LiveInfo()
        self._ok(self.L.sg_live_check(self.h, all_mask, fair, C.byref(li)))
        return _fields(li)

    def live_check_masked(self, all_mask, fair, kind, p, q):
        ci = LiveCheckInfo()
        self._ok(self.L.sg_live_check_masked(self.h, all_mask, fair, kind, p, q, C.byref(ci)))
        return _fields(ci)

    def live_trace(self, level_start):
        """(prefix, cycle) of the last check, as lists of states"""
        lv = np.ascontiguousarray(level_start, dtype=np.uint64)
        np_, nc = C.c_size_t(0), C.c_size_t(0)
        rc = self.L.sg_live_trace(self.h, _ptr(lv, C.c_uint64), len(lv), None, C.byref(np_), None, C.byref(nc))
        if rc != -1 or "buffers too small" not in self.L.sg_last_error().decode():   # MC_EBADCFG with the sizes: anything else is the answer
            self._ok(rc)
        prefix, cycle = np.empty(max(np_.value, 1), dtype=np.uint32), np.empty(max(nc.value, 1), dtype=np.uint32)
        self._ok(self.L.sg_live_trace(self.h, _ptr(lv, C.c_uint64), len(lv), _ptr(prefix, C.c_uint32), C.byref(np_), _ptr(cycle, C.c_uint32), C.byref(nc)))
        return prefix[:np_.value].tolist(), cycle[:nc.value].tolist()


def scan_exclusive_u32_to_u64(values, L=None):
    L = L or lib()
    a = np.ascontiguousarray(values, dtype=np.uint32)
    out = np.empty(len(a), dtype=np.uint64)
    rc = L.sg_scan_exclusive_u32_to_u64(_ptr(a, C.c_uint32), _ptr(out, C.c_uint64), len(a))
    if rc:
        raise SgError(rc, L.sg_last_error().decode())
    return out


def scan_answers_inclusive(answers, L=None):
    L = L or lib()
    a = np.ascontiguousarray(answers, dtype=np.uint8)
    out = np.empty(len(a), dtype=np.uint32)
    rc = L.sg_scan_answers_inclusive(_ptr(a, C.c_uint8), _ptr(out, C.c_uint32), len(a))
    if rc:
        raise SgError(rc, L.sg_last_error().decode())
    return out
