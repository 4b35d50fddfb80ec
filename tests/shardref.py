"""The host reference of tests/test_gpu_shard_steps.py: the breadth-first levels of a model, one state and one slot at a time, through
the host build of the lowerings (tests/_shim: shim_init_state, shim_eval_slot, shim_state_apply), and what ONE sharded expand of the
first level with at least min_frontier states must hand out on rank r of P.  tests/test_exchange_reference.py establishes on the CPU
that the chosen cases have what the GPU assertions need (CASES below)."""
import ctypes as C
import functools

import helpers

ST_ENABLED, ST_OUT_OF_MODEL, ST_ASSERT, ST_INVARIANT, ST_SPECERR, ST_OVERFLOW, ST_SELFLOOP = 1, 2, 4, 8, 16, 32, 64   # mc_common.h
MAX_SLOTS = 256          # a source word keeps the slot in 8 bits
SLOT_COPY = 0xfffc       # include/tlamc.h, mc_shard_fetch: the entry is a copy made by the replicated prefix

# (spec, params, P, r, min_frontier): the frontier is the first level with at least min_frontier states
CASES = {
    "raft-P1-r0": ("raft", [2, 2, 2, 9, 2, 1], 1, 0, 300),
    "raft-P3-r1": ("raft", [2, 2, 2, 9, 2, 1], 3, 1, 300),
    "raft-P8-r0": ("raft", [2, 2, 2, 9, 2, 1], 8, 0, 1000),
    "raft-P8-r7": ("raft", [2, 2, 2, 9, 2, 1], 8, 7, 1000),
    "ssi-P3-r1": ("ssi", [2, 2, 127, 0], 3, 1, 300),
}


def fp_owner(fp, P):
    """include/tlamc.h mc_fp_owner: the high bits pick the owner"""
    return 0 if P <= 1 else ((fp >> 40) * P) >> 24


class Host:
    """one model on the host: states are bytes of W words"""

    def __init__(self, spec, params):
        self.lib = L = helpers.shim_lib()
        self.d = helpers.spec_desc(spec, params)
        L.shim_state_bytes.restype = C.c_size_t
        L.shim_state_bytes.argtypes = [C.POINTER(helpers.McSpecDesc)]
        L.shim_init_state.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_uint64, C.c_char_p]
        L.shim_eval_slot.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_char_p, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint64)]
        L.shim_state_apply.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_char_p, C.c_int, C.c_char_p]
        L.shim_state_format.argtypes = [C.POINTER(helpers.McSpecDesc), C.c_char_p, C.c_char_p, C.c_size_t]
        self._text = C.create_string_buffer(1 << 16)
        self.nbytes = L.shim_state_bytes(C.byref(self.d))
        self.words = self.nbytes // 8

    def init(self, k):
        out = C.create_string_buffer(self.nbytes)
        assert self.lib.shim_init_state(C.byref(self.d), k, out) == 0
        return out.raw

    def eval(self, state, slot):
        """(status, fingerprint of the successor)"""
        st, fp = C.c_uint(0), C.c_uint64(0)
        assert self.lib.shim_eval_slot(C.byref(self.d), state, slot, C.byref(st), C.byref(fp)) == 0
        return st.value, fp.value

    def apply(self, state, slot):
        out = C.create_string_buffer(self.nbytes)
        assert self.lib.shim_state_apply(C.byref(self.d), state, slot, out) == 0
        return out.raw

    def key(self, state):
        """the state as TLA+ text: what two packed forms of ONE state have in common (raft keeps its messages in slots, in the order
        they were sent: two orders, one bag, one fingerprint)"""
        n = self.lib.shim_state_format(C.byref(self.d), state, self._text, len(self._text))
        assert 0 < n < len(self._text)
        return self._text.raw[:n]

    def candidates(self, state):
        """[(slot, fingerprint, successor)] of the successors that are candidates for the seen-set: enabled, inside the model, not the
        state itself"""
        out = []
        for slot in range(MAX_SLOTS):
            st, fp = self.eval(state, slot)
            if not st & ST_ENABLED:
                continue
            assert not st & (ST_ASSERT | ST_SPECERR | ST_OVERFLOW | ST_INVARIANT), "the cases are models that end without a finding"
            if st & (ST_OUT_OF_MODEL | ST_SELFLOOP):
                continue
            assert fp != 0
            out.append((slot, fp, self.apply(state, slot)))
        return out


@functools.lru_cache(maxsize=None)
def prefix(spec, params, min_frontier):
    """(host, levels: lists of states, {key: fingerprint} of every state but the initial ones): the search up to the first level
    with at least min_frontier states"""
    H = Host(spec, list(params))
    sizes = helpers.shim_run(spec, list(params))["levels"]
    levels, fps, seen = [[]], {}, set()
    for k in range(sizes[0]):
        s = H.init(k)
        if H.key(s) not in seen:
            seen.add(H.key(s))
            levels[0].append(s)
    while len(levels[-1]) < min_frontier:
        nxt = []
        for s in levels[-1]:
            for _, fp, t in H.candidates(s):
                k = H.key(t)
                if k not in seen:
                    seen.add(k)
                    fps[k] = fp
                    nxt.append(t)
                else:
                    assert fps.get(k, fp) == fp, "one state, two fingerprints"
        assert nxt, "the model ends before a level is this large"
        levels.append(nxt)
    assert [len(lv) for lv in levels] == sizes[:len(levels)], "the host search disagrees with the shim's own"
    return H, levels, fps


class Expected:
    """what rank r of P hands out when it expands `frontier` (packed states: its share of the last level of the prefix) once.  States are
    told apart by their TLA+ text (Host.key)."""

    def __init__(self, H, P, r, frontier, seen):
        self.H, self.P, self.r, self.frontier = H, P, r, list(frontier)
        self.cands = [H.candidates(s) for s in self.frontier]
        self.key_of = {}      # fingerprint -> key of the successor
        self.clash = False    # two different candidates with one fingerprint
        self.routed = [{} for _ in range(P)]   # per owner: fingerprint -> how many (state, slot) pairs generate it
        for cs in self.cands:
            for slot, fp, t in cs:
                self.clash |= self.key_of.setdefault(fp, H.key(t)) != H.key(t)
                owner = fp_owner(fp, P)
                self.routed[owner][fp] = self.routed[owner].get(fp, 0) + 1
        # the candidates this rank owns are probed here: new = not a state of the prefix (every rank's seen-set holds all of those)
        self.local_new = {self.key_of[fp] for fp in self.routed[r]} - set(seen)
        self.per_owner = [sum(c.values()) for c in self.routed]


def host_case(name):
    """(Expected on the host's own frontier, sizes of the prefix's levels, keys of the prefix, keys of rank r's share)"""
    spec, params, P, r, min_frontier = CASES[name]
    H, levels, fps = prefix(spec, tuple(params), min_frontier)
    seen = {H.key(s) for lv in levels for s in lv}
    share = [s for s in levels[-1] if fp_owner(fps[H.key(s)], P) == r]   # k_take_owned's share
    return Expected(H, P, r, share, seen), [len(lv) for lv in levels], seen, {H.key(s) for s in share}
