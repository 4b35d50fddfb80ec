"""tests/sfgraph.py's driver of the product's StateGraph with the two entries of the checks label by label
(tests/_ufgraph/ufgraph.hip, which includes tests/_sfgraph/sfgraph.hip whole, compiled together with tla_rust_amd/csrc/state_graph.hip
into a library of its own, without libtlamc.so).  Built on first use; hipcc cross-compiles gfx950 without a GPU."""
import ctypes as C

import numpy as np

import helpers
import sfgraph
import sgraph

SHIM_DIR = helpers.ROOT / "tests" / "_ufgraph"
CSRC = sgraph.CSRC


class FairUnits(C.Structure):
    """mc_fair_units"""
    _fields_ = [("nunits", C.c_int32), ("nconj", C.c_int32), ("of_unit", C.c_uint64 * 128), ("weak_mask", C.c_uint64), ("strong_mask", C.c_uint64)]


def fair_units(of_unit, nunits, nconj, weak, strong):
    fu = FairUnits()
    fu.nunits, fu.nconj, fu.weak_mask, fu.strong_mask = nunits, nconj, weak, strong
    for u, m in enumerate(of_unit):
        fu.of_unit[u] = m
    return fu


def build(csrc=None, out=None):
    """csrc: where state_graph.hip, engine_live.h and their headers are taken from (a copy with one edit is a mutant); out: where the
    library goes"""
    return sgraph.build_driver((out or SHIM_DIR / "_build") / "libufgraph.so", csrc or CSRC,
                               [SHIM_DIR / "ufgraph.hip", sfgraph.SHIM_DIR / "sfgraph.hip", sgraph.SHIM_DIR / "sgraph.hip"])


def load(so):
    L = sfgraph.load(so)
    vp = C.c_void_p
    L.uf_set_units.argtypes = [vp, C.POINTER(C.c_int8)]
    L.uf_destroy.argtypes = [vp]
    L.uf_destroy.restype = None
    L.uf_live_units.argtypes = [vp, C.POINTER(FairUnits), C.POINTER(sgraph.LiveInfo), C.POINTER(sfgraph.LiveStrongInfo)]
    L.uf_live_check_units.argtypes = [vp, C.POINTER(FairUnits), C.c_int, C.c_int, C.c_int, C.POINTER(sgraph.LiveCheckInfo), C.POINTER(sfgraph.LiveStrongInfo)]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build())
    return _lib


class Graph(sfgraph.Graph):
    """sfgraph.Graph over this library with the edges' units beside the edges' processes, plus the checks by units: each returns (the
    weak twin's fields, mc_live_strong_info's)"""

    def __init__(self, offsets, dst, proc, unit, pred=None, ninit=0, L=None):
        super().__init__(offsets, dst, proc, pred, ninit, L or lib())
        self._unit = np.ascontiguousarray(unit, dtype=np.int8)
        assert len(self._unit) == self.edges
        self._ok(self.L.uf_set_units(self.h, sgraph._ptr(self._unit, C.c_int8)))

    def close(self):
        if self.h:
            self.L.uf_destroy(self.h)
            self.h = None

    def live_units(self, fu):
        li, si = sgraph.LiveInfo(), sfgraph.LiveStrongInfo()
        self._ok(self.L.uf_live_units(self.h, C.byref(fu), C.byref(li), C.byref(si)))
        return sgraph._fields(li), sgraph._fields(si)

    def live_check_units(self, fu, kind, p, q):
        ci, si = sgraph.LiveCheckInfo(), sfgraph.LiveStrongInfo()
        self._ok(self.L.uf_live_check_units(self.h, C.byref(fu), kind, p, q, C.byref(ci), C.byref(si)))
        return sgraph._fields(ci), sgraph._fields(si)
