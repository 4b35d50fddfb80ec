"""Host walks of simulation mode (tests/_simshim: tla_rust_amd/csrc/sim_walk.h built with g++ over the spec lowerings, no HIP).

The library is built on first use (like helpers.build_shim); the PlusCal front-end it needs for compiled programs comes from
helpers' libshim.so, which it is linked against (not loaded with RTLD_GLOBAL: the shim's host stand-ins of the product's symbols would then
take the place of libtlamc's in every library loaded later, the generated-code engines of MC_F_JIT among them)."""
import ctypes as C

import helpers

SIMSHIM_DIR = helpers.ROOT / "tests" / "_simshim"
END = {1: "depth", 2: "violation", 3: "deadlock", 4: "out-of-model", 5: "stutter", 6: "overflow"}


class SimShimOut(C.Structure):
    _fields_ = [("generated", C.c_uint64), ("steps", C.c_uint64), ("walks", C.c_uint64), ("viol", C.c_uint64),
                ("max_depth", C.c_uint32), ("pad", C.c_uint32)]


def build_simshim(csrc=None, out=None):
    """the host walk library; csrc: the directory the lowerings and sim_walk.h are taken from (default: the product's; a copy of it
    with one edit is how tests/test_simulate_graph.py builds its mutants), out: where the library goes"""
    return helpers.build_over_shim((out or SIMSHIM_DIR / "_build") / "libsimshim.so", SIMSHIM_DIR / "simshim.cpp", csrc)


_lib = None


def load(so):
    L = C.CDLL(str(so))   # (its vm_make_params / vm_format of compiled programs: libshim.so's)
    L.simshim_walks.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_char_p, C.c_int,
                                C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint64),
                                C.POINTER(SimShimOut), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.simshim_format.argtypes = [C.POINTER(helpers.McSpecDesc), C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
    L.simshim_words.argtypes = [C.POINTER(helpers.McSpecDesc)]
    return L


def lib():
    global _lib
    if _lib is None:
        _lib = load(build_simshim())
    return _lib


NO_KEY = (1 << 64) - 1


def walks(spec, params, seed, n, depth, first=0, deadlock=True, dump=None, rows_walk=None, L=None):
    """host walks first .. first+n-1: dict(walks=[{len, end, slots, gen, viol}], generated, steps, walks_done, max_depth, viol, rows);
    L: a library from load() in place of the product's"""
    L = L or lib()
    d = helpers.spec_desc(spec, params)
    slots = (C.c_int32 * (n * depth))()
    ln = (C.c_uint32 * n)()
    en = (C.c_uint32 * n)()
    gen = (C.c_uint32 * n)()
    viol = (C.c_uint64 * n)()
    W = L.simshim_words(C.byref(d))
    rows = (C.c_uint64 * ((depth + 1) * W))() if rows_walk is not None else None
    o = SimShimOut()
    rc = L.simshim_walks(C.byref(d), seed, first, n, depth, int(deadlock), dump.encode() if dump else None, 1, slots, ln, en,
                         rows_walk if rows_walk is not None else 0, rows, C.byref(o), gen, viol)
    if rc:
        raise RuntimeError(f"simshim_walks: {rc}")
    ws = [dict(len=ln[k], end=en[k], slots=slots[k * depth:k * depth + max(ln[k] - 1, 0)], gen=gen[k],
               viol=None if viol[k] == NO_KEY else viol[k]) for k in range(n)]
    out = dict(walks=ws, generated=o.generated, steps=o.steps, walks_done=o.walks, max_depth=o.max_depth,
               viol=None if o.viol == NO_KEY else o.viol)
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


def key_inv(k):
    return (k >> 3) & 31


def oracle_levels(spec, params, path, check_deadlock=True):
    """{state text (one line): BFS level} of every state the oracle stores"""
    helpers.oracle_run(spec, params, check_deadlock=check_deadlock, stop=0, dump=str(path))
    lv = {}
    for level, texts in helpers.read_dump(str(path)).items():
        for t in texts:
            lv.setdefault(t, level)
    return lv


def _dump_lines(path):
    """[(tag, text)] of a host walk dump, whose lines name a text "#<id> <text>" where it first occurs and "#<id>" after that"""
    table, out = [], []
    with open(path) as f:
        for line in f:
            parts = line.rstrip("\n").split(" ", 2)
            if len(parts) == 3:
                assert int(parts[1][1:]) == len(table)
                table.append(parts[2])
            out.append((parts[0], table[int(parts[1][1:])]))
    return out


def walk_dump(path):
    """[(state number t, one-line text)] of the states reached, from a host walk dump"""
    return [(int(t[1:]), txt) for t, txt in _dump_lines(path) if t[0] == "S"]


def walk_texts(path, walks):
    """a host walk dump split by walk: [(texts of the states reached, text of the successor that broke an invariant or None)], one
    per entry of `walks` (walks()["walks"], whose lengths say where one walk's lines end)"""
    lines = _dump_lines(path)
    out, i = [], 0
    for w in walks:
        texts = []
        for t in range(1, w["len"] + 1):
            assert lines[i][0] == f"S{t}", (lines[i][0], t)
            texts.append(lines[i][1])
            i += 1
        succ = None
        if i < len(lines) and lines[i][0][0] == "V":
            assert lines[i][0] == f"V{w['len'] + 1}"
            succ = lines[i][1]
            i += 1
        out.append((texts, succ))
    assert i == len(lines)
    return out
