"""A test-only driver of the exchange half of the sharded engine (tests/_xchgshim/xchgshim.hip over tla_rust_amd/csrc/engine_kernels.h, a
library of its own without libtlamc.so): k_compact_buckets, k_compact_packed, k_gather_range_ends + k_compact_new, k_send_parents,
k_ingest, k_ingest_parents, k_bump_arena_next and k_gather_states on arrays that no search produced (tests/xchgmodel.py).  Built on first
use with the flags of tests/seenshim.py; hipcc cross-compiles gfx950 without a GPU, loading the library needs none either.
Every output is handed in pre-filled (FILL64 / FILL32 / ...) and comes back whole, so that a test compares the positions the kernel must
not write too; `intact` says that the guard zones around every written buffer are unchanged."""
import ctypes as C

import numpy as np

import helpers
import testlib

SHIM_DIR = helpers.ROOT / "tests" / "_xchgshim"
CSRC = helpers.ROOT / "tla_rust_amd" / "csrc"
NSHARD = 8                      # engine_kernels.h
DEV_EARENA, DEV_EROUTE = 2, 8   # engine_kernels.h: DEV_E*
FILL8, FILL16, FILL32, FILL64 = 0xa7, 0xa7a7, 0xa7a7a7a7, 0xa7a7a7a7a7a7a7a7   # what an output holds where nothing was written


def build(csrc=None, out=None):
    """csrc: the directory engine_kernels.h and the headers it needs are taken from (default: the product's; a copy with one edit is a
    mutant); out: where the library goes"""
    csrc = csrc or CSRC
    include = csrc.parent.parent / "include"   # (spec_registry.h includes ../../include/tlamc.h: a copy of csrc brings its own)
    return testlib.build_library((out or SHIM_DIR / "_build") / "libxchgshim.so", testlib.hip_argv("-I", include, "-I", csrc, SHIM_DIR / "xchgshim.hip"),
                                 [SHIM_DIR / "xchgshim.hip"] + testlib.product_deps(csrc))


_u64p, _u32p, _u16p, _u8p, _intp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), C.POINTER(C.c_int)


def load(so):
    L = C.CDLL(str(so))
    u64, u32 = C.c_uint64, C.c_uint
    L.xs_last_error.restype = C.c_char_p
    L.xs_compact_buckets.argtypes = [u32, _u64p, _u64p, _u32p, u64, u64, _u64p, _u32p, _intp]
    L.xs_compact_packed.argtypes = [u32, _u64p, _u64p, _u32p, u64, u64, _u64p, _u32p, _u32p, _intp]
    L.xs_compact_new.argtypes = [u32, _u8p, u64, _u64p, _u32p, _u32p, _u64p, _intp]
    L.xs_send_parents.argtypes = [u32, _u32p, u64, _u64p, _u64p, u64, _u64p, u64, _intp]
    L.xs_ingest.argtypes = [C.c_int, _u64p, u64, u64, u64, _u64p, u64, _u32p, _u64p, _u32p, _intp]
    L.xs_ingest_parents.argtypes = [_u64p, u64, u32, u64, u64, _u32p, _u16p, _u8p, _intp]
    L.xs_bump_arena_next.argtypes = [u64, u64, C.c_int, u64, _u64p, _u32p]
    L.xs_gather_states.argtypes = [C.c_int, _u64p, u64, u64, u64, _u64p, _intp]
    for name in ("xs_nshard", "xs_dev_earena", "xs_dev_eroute", "xs_guard"):
        getattr(L, name).restype = C.c_uint
    assert (L.xs_nshard(), L.xs_dev_earena(), L.xs_dev_eroute()) == (NSHARD, DEV_EARENA, DEV_EROUTE)
    assert L.xs_guard() >= 64
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load(build())
    return _lib


class XchgError(RuntimeError):
    pass


def _ok(L, rc):
    if rc:
        raise XchgError(f"{L.xs_last_error().decode()} (code {rc})")


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _p(a, ptype):
    return a.ctypes.data_as(ptype)


def compact_buckets(P, cursors, rt_fp, rt_src, subcap, L=None):
    """(send_fp, pend_src, intact): as long as the clamped cursors sum to"""
    L = L or lib()
    cursors, rt_fp, rt_src = _arr(cursors, np.uint64), _arr(rt_fp, np.uint64), _arr(rt_src, np.uint32)
    assert len(cursors) == P * NSHARD and len(rt_fp) == len(rt_src) == P * NSHARD * subcap
    n = int(np.minimum(cursors, np.uint64(subcap)).sum())
    fp, src, intact = np.full(max(n, 1), FILL64, dtype=np.uint64), np.full(max(n, 1), FILL32, dtype=np.uint32), C.c_int(0)
    _ok(L, L.xs_compact_buckets(P, _p(cursors, _u64p), _p(rt_fp, _u64p), _p(rt_src, _u32p), subcap, n, _p(fp, _u64p), _p(src, _u32p), C.byref(intact)))
    return fp[:n], src[:n], bool(intact.value)


def compact_packed(P, cursors, rt_fp, rt_src, subcap, cap, L=None):
    """(send_fp, pend_src: P * cap each, the error word, intact)"""
    L = L or lib()
    cursors, rt_fp, rt_src = _arr(cursors, np.uint64), _arr(rt_fp, np.uint64), _arr(rt_src, np.uint32)
    assert len(cursors) == P * NSHARD and len(rt_fp) == len(rt_src) == P * NSHARD * subcap
    fp, src = np.full(P * cap, FILL64, dtype=np.uint64), np.full(P * cap, FILL32, dtype=np.uint32)
    err, intact = C.c_uint32(0), C.c_int(0)
    _ok(L, L.xs_compact_packed(P, _p(cursors, _u64p), _p(rt_fp, _u64p), _p(rt_src, _u32p), subcap, cap, _p(fp, _u64p), _p(src, _u32p),
                               C.byref(err), C.byref(intact)))
    return fp, src, err.value, bool(intact.value)


def compact_new(P, answers, off, pend_src, L=None):
    """(new_src: as long as the answers, ends[P], intact)"""
    L = L or lib()
    answers, off, pend_src = _arr(answers, np.uint8), _arr(off, np.uint64), _arr(pend_src, np.uint32)
    total = len(answers)
    assert len(off) == 9 and len(pend_src) == total
    new_src, ends, intact = np.full(total, FILL32, dtype=np.uint32), np.zeros(P, dtype=np.uint64), C.c_int(0)
    _ok(L, L.xs_compact_new(P, _p(answers, _u8p), total, _p(off, _u64p), _p(pend_src, _u32p), _p(new_src, _u32p), _p(ends, _u64p), C.byref(intact)))
    return new_src, ends, bool(intact.value)


def send_parents(P, new_src, off, cnt, chunk_base, extra=3, L=None):
    """(send_parents: the sum of the counts and `extra` pre-filled words, intact)"""
    L = L or lib()
    new_src, off, cnt = _arr(new_src, np.uint32), _arr(off, np.uint64), _arr(cnt, np.uint64)
    assert len(off) == 9 and len(cnt) == P
    out, intact = np.full(int(cnt.sum()) + extra, FILL64, dtype=np.uint64), C.c_int(0)
    _ok(L, L.xs_send_parents(P, _p(new_src, _u32p), len(new_src), _p(off, _u64p), _p(cnt, _u64p), chunk_base, _p(out, _u64p), len(out), C.byref(intact)))
    return out, bool(intact.value)


def ingest(words, arena, arena_cap, arena_next, recv_blocks, n, parent, L=None):
    """shard_ingest's two kernels; arena and parent are written in place; (arena_next, the error word, intact)"""
    L = L or lib()
    recv_blocks = _arr(recv_blocks, np.uint64)
    assert arena.dtype == np.uint64 and parent.dtype == np.uint32 and arena.flags.c_contiguous and parent.flags.c_contiguous
    assert len(parent) == arena_cap and len(recv_blocks) == -(-n // 64) * 64 * words
    nxt, err, intact = C.c_uint64(0), C.c_uint32(0), C.c_int(0)
    _ok(L, L.xs_ingest(words, _p(arena, _u64p), arena.size, arena_cap, arena_next, _p(recv_blocks, _u64p), n, _p(parent, _u32p), C.byref(nxt),
                       C.byref(err), C.byref(intact)))
    return nxt.value, err.value, bool(intact.value)


def ingest_parents(recv_parents, src_rank, arena_next, parent, pslot, prank, L=None):
    """parent / pslot / prank are written in place; intact"""
    L = L or lib()
    recv_parents = _arr(recv_parents, np.uint64)
    assert parent.dtype == np.uint32 and pslot.dtype == np.uint16 and prank.dtype == np.uint8 and len(parent) == len(pslot) == len(prank)
    intact = C.c_int(0)
    _ok(L, L.xs_ingest_parents(_p(recv_parents, _u64p), len(recv_parents), src_rank, arena_next, len(parent), _p(parent, _u32p), _p(pslot, _u16p),
                               _p(prank, _u8p), C.byref(intact)))
    return bool(intact.value)


def bump_arena_next(arena_next, n, on_device, arena_cap, L=None):
    """(arena_next, the error word)"""
    L = L or lib()
    nxt, err = C.c_uint64(0), C.c_uint32(0)
    _ok(L, L.xs_bump_arena_next(arena_next, n, int(on_device), arena_cap, C.byref(nxt), C.byref(err)))
    return nxt.value, err.value


def gather_states(words, arena, first, count, L=None):
    """(count * words words, intact)"""
    L = L or lib()
    arena = _arr(arena, np.uint64)
    out, intact = np.full(count * words, FILL64, dtype=np.uint64), C.c_int(0)
    _ok(L, L.xs_gather_states(words, _p(arena, _u64p), len(arena), first, count, _p(out, _u64p), C.byref(intact)))
    return out, bool(intact.value)
