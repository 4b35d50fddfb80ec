"""Host walks of simulation mode (tests/_simshim: tla_rust_amd/csrc/sim_walk.h built with g++ over the spec lowerings, no HIP).

The library is built on first use (like helpers.build_shim); the PlusCal front-end it needs for compiled programs comes from
helpers' libshim.so, which it is linked against (not loaded with RTLD_GLOBAL: the shim's host stand-ins of the product's symbols would then
take the place of libtlamc's in every library loaded later, the generated-code engines of MC_F_JIT among them)."""
import ctypes as C
import fcntl
import os
import subprocess

import helpers

SIMSHIM_DIR = helpers.ROOT / "tests" / "_simshim"
END = {1: "depth", 2: "violation", 3: "deadlock", 4: "out-of-model", 5: "stutter", 6: "overflow"}


class SimShimOut(C.Structure):
    _fields_ = [("generated", C.c_uint64), ("steps", C.c_uint64), ("walks", C.c_uint64), ("viol", C.c_uint64),
                ("max_depth", C.c_uint32), ("pad", C.c_uint32)]


def build_simshim():
    out = SIMSHIM_DIR / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libsimshim.so"
    csrc = helpers.ROOT / "tla_rust_amd" / "csrc"
    shim = helpers.build_shim()
    srcs = [SIMSHIM_DIR / "simshim.cpp", shim] + list(csrc.glob("*.h")) + [helpers.ROOT / "include" / "tlamc.h"]

    def fresh():
        return so.exists() and all(so.stat().st_mtime >= s.stat().st_mtime for s in srcs)
    if fresh():
        return so
    with open(out / ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not fresh():
            tmp = out / f"libsimshim.{os.getpid()}.so"
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(tmp), str(SIMSHIM_DIR / "simshim.cpp"),
                            "-L", str(shim.parent), "-lshim", f"-Wl,-rpath,{shim.parent}"], check=True)
            os.replace(tmp, so)
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(str(build_simshim()))   # (its vm_make_params / vm_format of compiled programs: libshim.so's)
        L.simshim_walks.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_char_p,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint64),
                                    C.POINTER(SimShimOut)]
        L.simshim_format.argtypes = [C.POINTER(helpers.McSpecDesc), C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
        L.simshim_words.argtypes = [C.POINTER(helpers.McSpecDesc)]
        _lib = L
    return _lib


def walks(spec, params, seed, n, depth, first=0, deadlock=True, dump=None, rows_walk=None):
    """host walks first .. first+n-1: dict(walks=[{len, end, slots}], generated, steps, walks_done, max_depth, viol, rows)"""
    L = lib()
    d = helpers.spec_desc(spec, params)
    slots = (C.c_int32 * (n * depth))()
    ln = (C.c_uint32 * n)()
    en = (C.c_uint32 * n)()
    W = L.simshim_words(C.byref(d))
    rows = (C.c_uint64 * ((depth + 1) * W))() if rows_walk is not None else None
    o = SimShimOut()
    rc = L.simshim_walks(C.byref(d), seed, first, n, depth, int(deadlock), dump.encode() if dump else None, slots, ln, en,
                         rows_walk if rows_walk is not None else 0, rows, C.byref(o))
    if rc:
        raise RuntimeError(f"simshim_walks: {rc}")
    ws = [dict(len=ln[k], end=en[k], slots=[slots[k * depth + s] for s in range(max(ln[k] - 1, 0))]) for k in range(n)]
    out = dict(walks=ws, generated=o.generated, steps=o.steps, walks_done=o.walks, max_depth=o.max_depth,
               viol=None if o.viol == (1 << 64) - 1 else o.viol)
    if rows is not None:
        out["rows"] = [list(rows[k * W:(k + 1) * W]) for k in range(depth + 1)]
    return out


def fmt(spec, params, row):
    L = lib()
    d = helpers.spec_desc(spec, params)
    buf = C.create_string_buffer(1 << 16)
    n = L.simshim_format(C.byref(d), (C.c_uint64 * len(row))(*row), buf, len(buf))
    return buf.raw[:n].decode()


def key_walk(k):
    return k >> 24


def key_slot(k):
    return (k >> 8) & 0xffff


def key_kind(k):
    return k & 7


def oracle_levels(spec, params, path, check_deadlock=True):
    """{state text (one line): BFS level} of every state the oracle stores"""
    helpers.oracle_run(spec, params, check_deadlock=check_deadlock, stop=0, dump=str(path))
    lv = {}
    for level, texts in helpers.read_dump(str(path)).items():
        for t in texts:
            lv.setdefault(t, level)
    return lv


def walk_dump(path):
    """[(state number t, one-line text)] of a host walk dump"""
    out = []
    with open(path) as f:
        for line in f:
            t, txt = line.rstrip("\n").split(" ", 1)
            out.append((int(t[1:]), txt))
    return out
