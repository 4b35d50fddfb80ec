"""A test-only driver of the product's seen-set code (tests/_seenshim/seenshim.hip over tla_rust_amd/csrc/engine_kernels.h and graph.h, a
library of its own without libtlamc.so): the probers in every form, k_probe, k_probe_packed, k_insert and seen_find on fingerprints that no
model produced (tests/seenmodel.py).  Built on first use, like tests/sgraph.py's library; hipcc cross-compiles gfx950 without a GPU, loading
the library needs none either.  host_lib() is graph.h's seen_find alone, built with g++ and no HIP."""
import ctypes as C

import numpy as np

import helpers
import testlib

SHIM_DIR = helpers.ROOT / "tests" / "_seenshim"
CSRC = helpers.ROOT / "tla_rust_amd" / "csrc"
PLAIN, BLIND, PRE, SLOW, KPROBE = range(5)   # seenshim.hip: F_*
FORM_NAMES = {PLAIN: "plain", BLIND: "blind", PRE: "pre", SLOW: "slow", KPROBE: "k_probe"}
DEV_ETABLE = 1


def build(csrc=None, out=None):
    """csrc: the directory engine_kernels.h, graph.h and the headers they include are taken from (default: the product's; a copy with one
    edit is a mutant); out: where the library goes"""
    csrc = csrc or CSRC
    include = csrc.parent.parent / "include"   # (spec_registry.h includes ../../include/tlamc.h: a copy of csrc brings its own)
    return testlib.build_library((out or SHIM_DIR / "_build") / "libseenshim.so", testlib.hip_argv("-I", include, "-I", csrc, SHIM_DIR / "seenshim.hip"),
                                 [SHIM_DIR / "seenshim.hip"] + testlib.product_deps(csrc))


def build_host(csrc=None, out=None):
    """graph.h's seen_find over host memory: g++, no HIP"""
    csrc = csrc or CSRC
    return testlib.build_library((out or SHIM_DIR / "_build") / "libseenfind.so",
                                 testlib.host_argv("-O2", "-DSEENSHIM_HOST", "-I", csrc, "-x", "c++", SHIM_DIR / "seenshim.hip"),
                                 [SHIM_DIR / "seenshim.hip"] + testlib.product_deps(csrc))


_u64p, _u32p, _u16p, _u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)


def load(so):
    L = C.CDLL(str(so))
    u64 = C.c_uint64
    L.ss_last_error.restype = C.c_char_p
    L.ss_insert_keys.argtypes = [C.c_int, C.c_int, C.c_int, u64, _u64p, _u64p, u64, _u8p, _u32p, _u32p]
    L.ss_probe_packed.argtypes = [C.c_int, u64, _u64p, _u64p, u64, C.c_uint, _u8p, _u32p]
    L.ss_k_insert.argtypes = [C.c_int, u64, _u64p, _u64p, u64, u64, C.c_uint, C.c_uint, _u16p, _u32p, u64, _u64p]
    L.ss_find.argtypes = [C.c_int, u64, _u64p, _u64p, u64, _u64p]
    return L


def load_host(so):
    L = C.CDLL(str(so))
    L.ssh_find.argtypes = [_u64p, C.c_uint64, C.c_int, _u64p, C.c_uint64, _u64p]
    L.ssh_find.restype = None
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


class SeenError(RuntimeError):
    pass


def _ok(L, rc):
    if rc:
        raise SeenError(f"{L.ss_last_error().decode()} (code {rc})")


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _aligned_u64(a):
    """a copy on a 64-byte boundary (graph.h reads buckets with aligned loads)"""
    a = _u64(a)
    raw = np.empty(a.size * 8 + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    out = raw[off:off + a.size * 8].view(np.uint64)
    out[:] = a.reshape(-1)
    return out


def empty_table(nbuckets, slots):
    return np.zeros(nbuckets * slots, dtype=np.uint64)


def insert_keys(form, slots, nbuckets, table, keys, serial=False, L=None):
    """inserts into `table` in place; (answers as bool, per-key error bits, the counter block's error word)"""
    L = L or lib()
    keys = _u64(keys)
    assert table.dtype == np.uint64 and table.size == nbuckets * slots and table.flags.c_contiguous
    n = len(keys)
    ans, errs, cerr = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint32), C.c_uint32(0)
    _ok(L, L.ss_insert_keys(form, slots, int(serial), nbuckets, table.ctypes.data_as(_u64p), keys.ctypes.data_as(_u64p), n,
                            ans.ctypes.data_as(_u8p), errs.ctypes.data_as(_u32p), C.byref(cerr)))
    assert set(np.unique(ans[:n]).tolist()) <= {0, 1}, "an answer was not written"
    return ans[:n].astype(bool), errs[:n], cerr.value


def probe_packed(slots, nbuckets, table, fps, cap, nranks, L=None):
    """(answers as written: nranks * cap bytes over a 0xee pre-fill, the error word)"""
    L = L or lib()
    fps = _u64(fps)
    assert len(fps) == cap * nranks and table.size == nbuckets * slots
    ans, cerr = np.zeros(cap * nranks, dtype=np.uint8), C.c_uint32(0)
    _ok(L, L.ss_probe_packed(slots, nbuckets, table.ctypes.data_as(_u64p), fps.ctypes.data_as(_u64p), cap, nranks, ans.ctypes.data_as(_u8p), C.byref(cerr)))
    return ans, cerr.value


def k_insert(slots, nbuckets, table, cand, ncols, nsl, max_slots, newlist, L=None):
    """cand: (grid_y, row_stride) slot-major; newlist: pre-filled, written in place; (n_new, cells, error)"""
    L = L or lib()
    cand = _u64(cand)
    grid_y, row_stride = cand.shape
    nsl = np.ascontiguousarray(nsl, dtype=np.uint16)
    assert len(nsl) == ncols and newlist.dtype == np.uint32 and table.size == nbuckets * slots
    out = np.zeros(3, dtype=np.uint64)
    _ok(L, L.ss_k_insert(slots, nbuckets, table.ctypes.data_as(_u64p), cand.ctypes.data_as(_u64p), row_stride, ncols, grid_y, max_slots,
                         nsl.ctypes.data_as(_u16p), newlist.ctypes.data_as(_u32p), len(newlist), out.ctypes.data_as(_u64p)))
    return int(out[0]), int(out[1]), int(out[2])


def find(slots, nbuckets, table, keys, L=None):
    """seen_find on the device: positions (seenmodel.ABSENT = not stored)"""
    L = L or lib()
    keys, table = _u64(keys), _u64(table)
    pos = np.zeros(max(len(keys), 1), dtype=np.uint64)
    _ok(L, L.ss_find(slots, nbuckets, table.ctypes.data_as(_u64p), keys.ctypes.data_as(_u64p), len(keys), pos.ctypes.data_as(_u64p)))
    return pos[:len(keys)]


def host_find(slots, nbuckets, table, keys, L=None):
    """seen_find on the host"""
    L = L or host_lib()
    keys, table = _u64(keys), _aligned_u64(table)
    assert table.size == nbuckets * slots
    pos = np.zeros(max(len(keys), 1), dtype=np.uint64)
    L.ssh_find(table.ctypes.data_as(_u64p), nbuckets, int(slots != 8), keys.ctypes.data_as(_u64p), len(keys), pos.ctypes.data_as(_u64p))
    return pos[:len(keys)]
