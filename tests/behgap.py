"""Behaviour checking with unlogged steps (MC_BEH_F_HIDDEN) on the host and over the test lowering SpecGap (tests/_behshim/behgap.*).

hidden_check / hidden_path: behaviour.h's rule over a spec lowering with the hidden bits set (tests/_behshim/behshim.cpp takes the flags
word as it is; behgap.cpp adds beh_path).  GapModel: SpecGap's rows are (x, h) pairs; host(): the host rule, device(): the kernel
k_behaviours<SpecGap, MUTANT, true> of that library."""
import ctypes as C

import behshim
import helpers
import testlib
from behshim import STUTTER, Verdict

DIR = behshim.BEHSHIM_DIR
FULL = (1 << 64) - 1
ON_FOLD, ON_SPIN, ON_LEAK = 1, 2, 4
MUTANTS = (0, 4, 5, 6)


def flags_of(stutter=False, hidden=0):
    assert 0 <= hidden <= 255
    return (STUTTER if stutter else 0) | hidden << 8   # MC_BEH_F_STUTTER | MC_BEH_F_HIDDEN(hidden)


def hidden_check(m, rows_list, mask=None, stutter=False, hidden=0):
    """behshim.Model.check with the hidden bits: the verdicts of a batch as dicts"""
    first, blob = m._batch(rows_list, mask)
    out = (Verdict * max(len(rows_list), 1))()
    rc = m.L.behshim_check(C.byref(m.d), len(rows_list), first, blob, mask, flags_of(stutter, hidden), out)
    assert rc == 0, rc
    return [v.as_dict() for v in out[:len(rows_list)]]


def build_host(csrc=None, out=None):
    """behgap.cpp with g++ (csrc: the product's headers, or a copy with one line of behaviour.h edited)"""
    return helpers.build_over_shim((out or DIR / "_build") / "libbehgap.so", DIR / "behgap.cpp", csrc, more=["-I", DIR], deps=[DIR / "behgap.h"])


_GAP_ARGS = [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int]


def load_host(so):
    L = C.CDLL(str(so))
    D = C.POINTER(helpers.McSpecDesc)
    L.behgap_path.argtypes = [D, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint, C.POINTER(Verdict), C.c_char_p, C.POINTER(C.c_int32),
                              C.POINTER(C.c_uint32), C.c_size_t]
    L.behgap_path.restype = C.c_long
    L.bg_host.argtypes = _GAP_ARGS + [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint, C.POINTER(Verdict)]
    L.bg_path.argtypes = _GAP_ARGS + [C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64), C.c_uint, C.POINTER(Verdict), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_size_t]
    L.bg_path.restype = C.c_long
    return L


_host = None


def host_lib():
    global _host
    if _host is None:
        _host = load_host(build_host())
    return _host


def hidden_path(m, rows, mask=None, stutter=False, hidden=0, L=None):
    """(verdict, [(slot, row, obs)]) of one behaviour: what mc_engine_behaviour_path gives"""
    L = L or host_lib()
    cap = len(rows) * (hidden + 1)
    v, states, slots, obs = Verdict(), C.create_string_buffer(cap * m.W), (C.c_int32 * cap)(), (C.c_uint32 * cap)()
    n = L.behgap_path(C.byref(m.d), b"".join(rows), len(rows), mask, flags_of(stutter, hidden), C.byref(v), states, slots, obs, cap)
    assert n >= 0   # (n <= (H + 1) * step <= cap)
    return v.as_dict(), [(slots[k], states.raw[k * m.W:(k + 1) * m.W], obs[k]) for k in range(n)]


# ------------------------------------------------------------------------------------------------ the kernel over SpecGap
def build_device(mutant=0):
    """tests/_behshim/behgap.hip for gfx950: mutant 0 is the product's kernel, 4 / 5 / 6 the kernel with one thing broken"""
    src = DIR / "behgap.hip"
    return testlib.build_library(DIR / "_build" / f"libbehgapdev{mutant}.so",
                                 testlib.hip_argv(f"-DBEH_MUTANT={mutant}", "-I", helpers.ROOT / "include", "-I", testlib.CSRC, "-I", DIR, src),
                                 [src, DIR / "behgap.h"] + testlib.product_deps(testlib.CSRC))


def build_devices():
    return list(testlib.build_mutants(MUTANTS, build_device).values())


class GapModel:
    """SpecGap: a case is (K, h0, G, B, on); a batch is a list of behaviours, each a list of (x, h) rows"""

    def __init__(self, mutant=None):
        """mutant None: the host library alone (no HIP)"""
        self.mutant = mutant
        if mutant is None:
            self.L = host_lib()
        else:
            self.L = C.CDLL(str(build_device(mutant)))
            self.L.bg_host.argtypes = host_lib().bg_host.argtypes
            self.L.bg_device.argtypes = self.L.bg_host.argtypes[:-1] + [C.c_uint32, C.POINTER(Verdict)]
            self.L.bg_last_error.restype = C.c_char_p
            assert self.L.bg_mutant() == mutant

    @staticmethod
    def _args(case, batch, mask, stutter, hidden):
        first = (C.c_uint64 * (len(batch) + 1))()
        flat = []
        for b, rows in enumerate(batch):
            first[b + 1] = first[b] + len(rows)
            flat += [w for r in rows for w in r]
        m = (C.c_uint64 * 2)(*mask) if mask is not None else None
        return [*case, len(batch), first, (C.c_uint64 * len(flat))(*flat), m, flags_of(stutter, hidden)], (Verdict * len(batch))()

    def host(self, case, batch, mask=None, stutter=False, hidden=0):
        a, out = self._args(case, batch, mask, stutter, hidden)
        assert self.L.bg_host(*a, out) == 0
        return [v.as_dict() for v in out]

    def device(self, case, batch, mask=None, stutter=False, hidden=0, iters=3):
        a, out = self._args(case, batch, mask, stutter, hidden)
        rc = self.L.bg_device(*a, iters, out)
        assert rc == 0, (rc, self.L.bg_last_error())
        return [v.as_dict() for v in out]

    def path(self, case, rows, mask=None, stutter=False, hidden=0):
        """(verdict, [(slot, (x, h), obs)]) on the host"""
        cap = len(rows) * (hidden + 1)
        flat = [w for r in rows for w in r]
        v, states, slots, obs = Verdict(), (C.c_uint64 * (2 * cap))(), (C.c_int32 * cap)(), (C.c_uint32 * cap)()
        m = (C.c_uint64 * 2)(*mask) if mask is not None else None
        n = host_lib().bg_path(*case, (C.c_uint64 * len(flat))(*flat), len(rows), m, flags_of(stutter, hidden), C.byref(v), states, slots, obs, cap)
        assert n >= 0
        return v.as_dict(), [(slots[k], (states[2 * k], states[2 * k + 1]), obs[k]) for k in range(n)]


X_ONLY = (FULL, 0)


def v(verdict, step, candidates, peak, generated, outside=0, errors=0):
    return dict(verdict=verdict, step=step, candidates=candidates, peak=peak, generated=generated, outside=outside, errors=errors)


def xs(*values):
    """a log of x alone"""
    return [(x, 0) for x in values]


# name: ((K, h0, G, B, on), batch, H, iters, what the rule gives — worked out by hand from behgap.h's table)
GAP_CASES = {
    # K_0 = {(0,0)}; h climbs 0 -> 1 -> 2 -> 3 through `work`, one row per depth, then `tick`.  Per member: h < 3 one slot, h = 3 one.
    "exactly G hidden steps, H = G": ((1, 0, 3, 0, 0), [xs(0, 1)], 3, 3, [v("accepted", 2, 1, 4, 1 + 4)]),
    "exactly G hidden steps, H = G - 1": ((1, 0, 3, 0, 0), [xs(0, 1)], 2, 3, [v("rejected", 1, 1, 3, 1 + 3)]),
    # G = 0: `tick` from h = 0 only, `work` never; `spin` 0 <-> 1.  The closure is {0, 1} whatever H is; 3 successors evaluated.
    "a hidden two-cycle": ((1, 0, 0, 0, ON_SPIN), [xs(0, 1)], 70, 3, [v("accepted", 2, 1, 2, 1 + 2 + 1)]),
    # K_0 = h 32 .. 63; `fold` gives 16 .. 31, each from two neighbouring lanes; depth 1 (= H) is evaluated and adds nothing: 16 folds,
    # 4 works (h < 20) and the one tick from h = 20
    "neighbouring lanes bring one closure row": ((32, 32, 20, 0, ON_FOLD), [xs(0, 1)], 1, 3, [v("accepted", 2, 1, 48, 32 + 32 + 16 + 4 + 1)]),
    # 63 fresh rows behind the one member: 64.  Depth 0: 63 + tick; depth 1: 63 members of 63 slots each.
    "a closure of exactly 64": ((1, 0, 0, 63, 0), [xs(0, 1)], 1, 3, [v("accepted", 2, 1, 64, 1 + 64 + 63 * 63)]),
    # 64 fresh rows: 65.  The member of depth 0 is evaluated (64 + tick), then the observation ends
    "a closure of 65": ((1, 0, 0, 64, 0), [xs(0, 1)], 1, 3, [v("ambiguous", 1, 1, 1, 1 + 65)]),
    # two logged states that agree on x: (0,1) is a successor of K_0 that matches o_0 and o_1 — it joins C and K_1; (0,2), from the
    # closure member (0,1), joins K_1 only.  Then C_2 = {1, 2, 3?}: G = 2, so h stops at 2: C_2 = {(0,1), (0,2)}, tick from h = 2.
    "a row that joins C and K at once": ((1, 0, 2, 0, 0), [xs(0, 0, 1)], 1, 3, [v("accepted", 3, 1, 2, 1 + (1 + 1) + (1 + 1))]),
    # seven observations, two hidden steps in every gap, launches of 3 observations: the gaps into observations 3 and 6 begin with a
    # carried set.  Each gap: h = 0, 1 (work), h = 2 (tick).
    "a gap that straddles a launch boundary": ((1, 0, 2, 0, 0), [xs(0, 1, 2, 3, 4, 5, 6), xs(0, 1, 2, 3)], 2, 3,
                                               [v("accepted", 7, 1, 3, 1 + 6 * 3), v("accepted", 4, 1, 3, 1 + 3 * 3)]),
    # `leak` changes x by 2 and `tick` by 1: x = 0, 3 has no path whose intermediate states all show x = 0
    "an internal step that touches the logged word": ((1, 0, 0, 0, ON_LEAK), [xs(0, 3)], 1, 3, [v("rejected", 1, 1, 1, 1 + 2)]),
}
MUTANT_CASE = {4: "a hidden two-cycle", 5: "exactly G hidden steps, H = G - 1", 6: "an internal step that touches the logged word"}
