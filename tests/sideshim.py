"""A test-only driver of the side passes that are templated on a lowering (tests/_sideshim/sideshim.hip over engine_graph.h,
engine_coverage.h and engine_violations.h with the table lowering of tests/_sideshim/spec_table.h; a library of its own without
libtlamc.so): the CSR build with k_live_proc / k_live_unit / k_live_pred, the two coverage histograms and the two -continue passes, on
rows that no search produced (tests/sidemodel.py).  Built on first use with the flags of tests/seenshim.py; hipcc cross-compiles gfx950
without a GPU, loading the library needs none either.  host_lib() is tests/_sideshim/sidehost.cpp: the product's HOST loops over the same
lowering, g++ and no HIP, with the same outputs.
Outputs the engine clears itself (slot_index, degree, pred) come back as the passes left them; every other output is handed in
pre-filled (FILL*) and comes back whole, so that a test compares the positions a kernel must not write too; `intact` says that the guard
zones around every written buffer are unchanged."""
import ctypes as C

import numpy as np

import helpers
import testlib
from seenshim import _aligned_u64

SHIM_DIR = helpers.ROOT / "tests" / "_sideshim"
CSRC = helpers.ROOT / "tla_rust_amd" / "csrc"
FILL8, FILL16, FILL32 = 0x57, 0x5757, 0x57575757   # what an output holds where nothing was written (positive as int8 / int16 too)
COV_MAX_BINS, VIOL_BINS, SPARSE_SLOTS = 512, 34, 4  # coverage.h, violations.h, graph.h
HEAD = 4                                            # spec_table.h: words of a row in front of the slots


class Params(C.Structure):
    _fields_ = [("max_slots", C.c_int), ("nbins", C.c_int), ("ninst", C.c_int), ("maxch", C.c_int)]


def words(prm):
    return HEAD + 2 * prm.max_slots


def build(csrc=None, out=None):
    """csrc: the directory the product's headers are taken from (default: the product's; a copy with one edit is a mutant); out: where
    the library goes"""
    csrc = csrc or CSRC
    include = csrc.parent.parent / "include"   # (spec_registry.h includes ../../include/tlamc.h: a copy of csrc brings its own)
    return testlib.build_library((out or SHIM_DIR / "_build") / "libsideshim.so",
                                 testlib.hip_argv("-I", include, "-I", csrc, "-I", SHIM_DIR, SHIM_DIR / "sideshim.hip"),
                                 [SHIM_DIR / "sideshim.hip", SHIM_DIR / "spec_table.h"] + testlib.product_deps(csrc))


def build_host(csrc=None, out=None):
    csrc = csrc or CSRC
    return testlib.build_library((out or SHIM_DIR / "_build") / "libsidehost.so", testlib.host_argv("-O2", "-I", csrc, "-I", SHIM_DIR, SHIM_DIR / "sidehost.cpp"),
                                 [SHIM_DIR / "sidehost.cpp", SHIM_DIR / "spec_table.h"] + testlib.product_deps(csrc))


_u64p, _u32p, _u16p, _i16p, _i8p, _intp = (C.POINTER(t) for t in (C.c_uint64, C.c_uint32, C.c_uint16, C.c_int16, C.c_int8, C.c_int))
_prmp, u64 = C.POINTER(Params), C.c_uint64
_GRAPH_OUT = [_u32p, _u32p, _u64p, _u32p, _i16p, _i8p, _i8p, _u32p, _u64p, _u64p, _u64p, _u64p]


def load(so):
    L = C.CDLL(str(so))
    L.sd_last_error.restype = C.c_char_p
    L.sd_graph.argtypes = [_prmp, _u64p, u64, u64, _u64p, u64, C.c_int, u64, _i8p, C.c_int, C.c_int, u64] + _GRAPH_OUT + [_intp]
    L.sd_coverage.argtypes = [_prmp, _u64p, u64, _u32p, _u16p, u64, u64, u64, u64, u64, _u64p, _intp]
    L.sd_violations.argtypes = [C.c_int, _prmp, _u64p, u64, _u32p, _u16p, u64, u64, u64, C.c_int, C.c_uint, u64, _u64p, _intp]
    for name in ("sd_guard", "sd_cov_max_bins", "sd_viol_bins", "sd_sparse_slots"):
        getattr(L, name).restype = C.c_uint
    assert (L.sd_cov_max_bins(), L.sd_viol_bins(), L.sd_sparse_slots()) == (COV_MAX_BINS, VIOL_BINS, SPARSE_SLOTS) and L.sd_guard() >= 64
    return L


def load_host(so):
    L = C.CDLL(str(so))
    L.sh_graph.argtypes = [_prmp, _u64p, u64, u64, _u64p, u64, C.c_int, _i8p, C.c_int, C.c_int, u64] + _GRAPH_OUT
    L.sh_coverage.argtypes = [_prmp, _u64p, u64, _u32p, _u16p, u64, u64, u64, u64, _u64p]
    L.sh_violations.argtypes = [C.c_int, _prmp, _u64p, u64, _u32p, _u16p, u64, u64, u64, C.c_int, C.c_uint, _u64p]
    return L


_lib = _host = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build())
    return _lib


def host_lib():
    global _host
    if _host is None:
        _host = load_host(build_host())
    return _host


class SideError(RuntimeError):
    pass


def _ok(L, rc):
    if rc:
        raise SideError(f"{L.sd_last_error().decode()} (code {rc})")


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _p(a, ptype):
    return a.ctypes.data_as(ptype)


def _rows(prm, rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    assert rows.ndim == 2 and rows.shape[1] == words(prm) and len(rows) >= 1
    return rows.reshape(-1), rows.shape[0]


def graph(prm, rows, expanded, table, nbuckets, sparse, chunk, unit_tab, nlabels, npred, cap, L=None, host=False):
    """The CSR build and the three liveness columns.  A dict: slot_index, degree, offsets, dst, act, proc, unit (cap elements each,
    pre-filled), pred, gc_degree and gc_fill (missing_states, missing_succ, first_bad, dropped, self_loops, max_degree), pred_bad, edges,
    intact.  host: tests/_sideshim/sidehost.cpp's loops instead of the kernels (chunk has no meaning there)."""
    flat, n = _rows(prm, rows)
    slots = SPARSE_SLOTS if sparse else 8
    table = _aligned_u64(table)
    assert table.size == nbuckets * slots
    unit_tab = _arr(unit_tab, np.int8)
    assert len(unit_tab) == max(prm.ninst, 1) * nlabels
    o = dict(slot_index=np.full(nbuckets * slots, FILL32, np.uint32), degree=np.full(n + 1, FILL32, np.uint32), offsets=np.zeros(n + 1, np.uint64),
             dst=np.full(cap, FILL32, np.uint32), act=np.full(cap, FILL16, np.int16), proc=np.full(cap, FILL8, np.int8), unit=np.full(cap, FILL8, np.int8),
             pred=np.full(n, FILL32, np.uint32), gc_degree=np.zeros(6, np.uint64), gc_fill=np.zeros(6, np.uint64))
    pred_bad, edges, intact = u64(0), u64(0), C.c_int(1 if host else 0)
    outs = [_p(o["slot_index"], _u32p), _p(o["degree"], _u32p), _p(o["offsets"], _u64p), _p(o["dst"], _u32p), _p(o["act"], _i16p), _p(o["proc"], _i8p),
            _p(o["unit"], _i8p), _p(o["pred"], _u32p), _p(o["gc_degree"], _u64p), _p(o["gc_fill"], _u64p), C.byref(pred_bad), C.byref(edges)]
    if host:
        L = L or host_lib()
        rc = L.sh_graph(C.byref(prm), _p(flat, _u64p), n, expanded, _p(table, _u64p), nbuckets, int(sparse), _p(unit_tab, _i8p), nlabels, npred, cap, *outs)
        assert rc == 0, "the outputs do not hold the edges"
    else:
        L = L or lib()
        _ok(L, L.sd_graph(C.byref(prm), _p(flat, _u64p), n, expanded, _p(table, _u64p), nbuckets, int(sparse), chunk, _p(unit_tab, _i8p), nlabels, npred, cap,
                          *outs, C.byref(intact)))
    o.update(pred_bad=pred_bad.value, edges=edges.value, intact=bool(intact.value))
    return o


def coverage(prm, rows, parent, pslot, gen_lo, gen_hi, dist_lo, dist_hi, chunk, bins, L=None, host=False):
    """(bins: 2 * nbins counters, generated then distinct, added to a copy of what was handed in; intact)"""
    flat, n = _rows(prm, rows)
    parent, pslot, bins = _arr(parent, np.uint32), _arr(pslot, np.uint16), _arr(bins, np.uint64).copy()
    assert len(parent) == len(pslot) == n and len(bins) == 2 * prm.nbins
    intact = C.c_int(1 if host else 0)
    if host:
        L = L or host_lib()
        L.sh_coverage(C.byref(prm), _p(flat, _u64p), n, _p(parent, _u32p), _p(pslot, _u16p), gen_lo, gen_hi, dist_lo, dist_hi, _p(bins, _u64p))
    else:
        L = L or lib()
        _ok(L, L.sd_coverage(C.byref(prm), _p(flat, _u64p), n, _p(parent, _u32p), _p(pslot, _u16p), gen_lo, gen_hi, dist_lo, dist_hi, chunk, _p(bins, _u64p),
                             C.byref(intact)))
    return bins, bool(intact.value)


def violations(stored, prm, rows, parent, pslot, lo, hi, new_hi, expanded, flags, chunk, bins, L=None, host=False):
    """(ViolBins as 4 * VIOL_BINS words: count[2 * VIOL_BINS], first[2 * VIOL_BINS], accumulated into a copy of what was handed in; intact)"""
    flat, n = _rows(prm, rows)
    parent, pslot, bins = _arr(parent, np.uint32), _arr(pslot, np.uint16), _arr(bins, np.uint64).copy()
    assert len(parent) == len(pslot) == n and len(bins) == 4 * VIOL_BINS
    intact = C.c_int(1 if host else 0)
    if host:
        L = L or host_lib()
        L.sh_violations(int(stored), C.byref(prm), _p(flat, _u64p), n, _p(parent, _u32p), _p(pslot, _u16p), lo, hi, new_hi, int(expanded), flags, _p(bins, _u64p))
    else:
        L = L or lib()
        _ok(L, L.sd_violations(int(stored), C.byref(prm), _p(flat, _u64p), n, _p(parent, _u32p), _p(pslot, _u16p), lo, hi, new_hi, int(expanded), flags, chunk,
                               _p(bins, _u64p), C.byref(intact)))
    return bins, bool(intact.value)
