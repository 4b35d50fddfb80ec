"""tests/sgraph.py's driver of the product's StateGraph with the two entries of the checks under strong fairness
(tests/_sfgraph/sfgraph.hip, which includes tests/_sgraph/sgraph.hip whole, compiled together with tla_rust_amd/csrc/state_graph.hip into
a library of its own, without libtlamc.so).  Built on first use; hipcc cross-compiles gfx950 without a GPU."""
import ctypes as C

import helpers
import sgraph

SHIM_DIR = helpers.ROOT / "tests" / "_sfgraph"
CSRC = sgraph.CSRC


class LiveStrongInfo(C.Structure):
    """mc_live_strong_info"""
    _fields_ = [("rounds", C.c_uint32), ("scc_builds", C.c_uint32), ("closed_states", C.c_uint64), ("final_components", C.c_uint64),
                ("seconds", C.c_double)]


def build(csrc=None, out=None):
    """csrc: where state_graph.hip, engine_live.h and their headers are taken from (a copy with one edit is a mutant); out: where the
    library goes"""
    return sgraph.build_driver((out or SHIM_DIR / "_build") / "libsfgraph.so", csrc or CSRC, [SHIM_DIR / "sfgraph.hip", sgraph.SHIM_DIR / "sgraph.hip"])


def load(so):
    L = sgraph.load(so)
    u64, vp = C.c_uint64, C.c_void_p
    L.sf_live_strong.argtypes = [vp, u64, u64, u64, C.POINTER(sgraph.LiveInfo), C.POINTER(LiveStrongInfo)]
    L.sf_live_check_strong.argtypes = [vp, u64, u64, u64, C.c_int, C.c_int, C.c_int, C.POINTER(sgraph.LiveCheckInfo), C.POINTER(LiveStrongInfo)]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build())
    return _lib


class Graph(sgraph.Graph):
    """sgraph.Graph over this library, plus the strong checks: each returns (the weak twin's fields, mc_live_strong_info's)"""

    def __init__(self, offsets, dst, proc=None, pred=None, ninit=0, L=None):
        super().__init__(offsets, dst, proc, pred, ninit, L or lib())

    def live_strong(self, all_mask, weak, strong):
        li, si = sgraph.LiveInfo(), LiveStrongInfo()
        self._ok(self.L.sf_live_strong(self.h, all_mask, weak, strong, C.byref(li), C.byref(si)))
        return sgraph._fields(li), sgraph._fields(si)

    def live_check_strong(self, all_mask, weak, strong, kind, p, q):
        ci, si = sgraph.LiveCheckInfo(), LiveStrongInfo()
        self._ok(self.L.sf_live_check_strong(self.h, all_mask, weak, strong, kind, p, q, C.byref(ci), C.byref(si)))
        return sgraph._fields(ci), sgraph._fields(si)
