"""The sharded step calls (include/tlamc.h mc_shard_*, Engine.shard_* of tla_rust_amd/binding.py) one by one, on real states: one engine
is rank r of P, the test plays the other ranks, and a host reference (tests/shardref.py over tests/_shim: one state and one slot at a
time) says what every call must hand out.  Every comparison is exact.

What the code says about duplicates (engine_kernels.h, k_expand_insert / k_expand_family): a wavefront drops a candidate whose
fingerprint it has queued before (the duplicate filter in front of the seen-set: raft's by-family kernel always, the slot-by-slot kernel
for specs with WAVE_FILTER), in route mode too, so the same fingerprint from two (state, slot) pairs reaches an owner's range once or
twice depending on which wavefront met it.  The exact and the packed form are therefore compared as SETS of fingerprints (and no
fingerprint more often than pairs generate it); with MC_F_NOFILTER nothing is dropped before routing and the MULTISET is compared.
Everything behind the routing is positional and compared element by element.

raft keeps its messages in slots in the order they were sent, so one state has several packed forms (one TLA+ text, one fingerprint):
a state is identified by its text (shardref.Host.key), and byte for byte through the parent the engine names for it."""
import collections

import numpy as np
import pytest
import torch

import shardref as R
import xchgmodel as M
from tla_rust_amd import binding as B

pytestmark = pytest.mark.gpu

MC_F_NOFILTER = 8192   # include/tlamc.h
MC_EROUTE = -10
FILL = np.uint64(M.FILL64).astype(np.int64).item()


class Rank:
    """one engine as rank r of P, at the start of the first sharded level"""

    def __init__(self, name, flags=0):
        self.spec, self.params, self.P, self.r, min_frontier = R.CASES[name]
        self.host, self.sizes, self.seen, self.share = host(name)
        self.H = self.host.H
        self.eng = B.Engine(self.spec, self.params, table_capacity=1 << 20, arena_capacity=1 << 18, chunk_states=1 << 12, trace=True,
                            shard_rank=self.r, shard_count=self.P, debug_flags=flags)
        self.levels = self.eng.shard_begin_replicated(min_frontier)
        self.n0, self.nloc = sum(self.levels), self.eng.shard_level_size()
        self.W = self.H.words

    def close(self):
        self.eng.close()

    def fetch(self, idx):
        """(state, parent rank, parent index, parent slot)"""
        return self.eng.shard_fetch(idx)

    def arena_next(self):
        """mc_shard_counters' distinct_local leaves out what another rank counts: the prefix on every rank but 0, the copies on all"""
        return self.eng.shard_counters()[1] + (self.nloc if self.r == 0 else self.n0 + self.nloc)

    def frontier(self):
        return [self.fetch(self.n0 + j)[0] for j in range(self.nloc)]

    def expected(self):
        return R.Expected(self.H, self.P, self.r, self.frontier(), self.seen)

    def check_step(self, state, parent, front):
        """the entry's parent is a state of the local frontier, and the slot it names leads to exactly these bytes"""
        prank, pidx, pslot = parent
        assert prank == self.r and self.n0 <= pidx < self.n0 + self.nloc
        assert self.H.apply(front[pidx - self.n0], pslot) == state


_host = {}


def host(name):
    if name not in _host:   # (the prefix search behind it is shared by the cases of one model)
        _host[name] = R.host_case(name)
    return _host[name]


@pytest.fixture
def rank(request):
    made = []

    def make(name, flags=0):
        assert not made, "one engine at a time"
        made.append(Rank(name, flags))
        return made[-1]
    yield make
    for k in made:
        k.close()


def device(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def filled(n):
    t = torch.full((max(n, 1),), FILL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def words(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64 if t.dtype == torch.int64 else np.uint8)


def check_conditions(E, P, r):
    """what the cases were chosen for (tests/test_exchange_reference.py establishes the same on the CPU)"""
    remote = [n for t, n in enumerate(E.per_owner) if t != r]
    assert P == 1 or sum(n > 64 for n in remote) >= 2
    assert any(n % 64 for n in E.per_owner)
    assert not E.clash


def check_routed(E, fps, counts, exact):
    """fps: per owner what its range holds"""
    for t in range(E.P):
        assert len(fps[t]) == counts[t]
        if t == E.r:
            assert counts[t] == 0   # its candidates were probed here
            continue
        got = collections.Counter(int(f) for f in fps[t])
        assert set(got) == set(E.routed[t]), f"owner {t}"
        assert all(got[f] <= E.routed[t][f] for f in got), f"owner {t}"
        if exact:
            assert got == collections.Counter(E.routed[t]), f"owner {t}"


def expand_exact(k, send_cap=1 << 15):
    """(send_fp, counts, offsets)"""
    send_fp = filled(send_cap)
    k.eng.shard_expand_launch(0, 0, k.nloc, send_cap)
    counts = k.eng.shard_expand_finish(0, send_fp.data_ptr(), send_cap)
    fp = words(send_fp)
    total = sum(counts)
    assert (fp[total:] == M.FILL64).all() and (fp[:total] != 0).all()
    return send_fp, fp[:total], counts, M.offsets(k.P, counts)


def check_local_new(k, E, front, a0):
    """the locally owned new states behind arena index a0; returns where they end"""
    a1 = k.arena_next()
    entries = [k.fetch(i) for i in range(a0, a1)]
    keys = [k.H.key(e[0]) for e in entries]
    assert len(keys) == len(set(keys)) and set(keys) == E.local_new
    for e in entries:
        k.check_step(e[0], e[1:], front)
    return a1


# ------------------------------------------------------------------------------------------------------------------- the local frontier
@pytest.mark.parametrize("name", list(R.CASES))
def test_local_frontier(rank, name):
    """mc_shard_begin_replicated: rank r holds copies of exactly the states of the level that it owns (k_take_owned)"""
    k = rank(name)
    assert k.levels == k.sizes
    assert k.nloc == len(k.share)
    _, _, fps = R.prefix(k.spec, tuple(k.params), R.CASES[name][4])
    keys = set()
    for j in range(k.nloc):
        state, prank, pidx, pslot = k.fetch(k.n0 + j)
        assert pslot == R.SLOT_COPY and prank == k.r and k.n0 - k.levels[-1] <= pidx < k.n0
        assert k.fetch(pidx)[0] == state
        assert B.lib().mc_fp_owner(fps[k.H.key(state)], k.P) == k.r == R.fp_owner(fps[k.H.key(state)], k.P)
        keys.add(k.H.key(state))
    assert keys == k.share   # ... all of them, none twice: the others are the complement
    assert k.arena_next() == k.n0 + k.nloc


# ---------------------------------------------------------------------------------------------------------------------- the exact form
def answer_vectors(lengths, seed):
    """the crafted vectors of tests/xchgmodel.py over the real ranges, and the block-plan counts where a range is long enough"""
    rng = np.random.default_rng(seed)
    vecs = dict(M.answer_patterns(lengths, rng))
    for shift in (0, 3):
        want = [min(M.BLOCK_COUNTS[(t + shift) % len(M.BLOCK_COUNTS)], n) for t, n in enumerate(lengths)]
        vecs[f"counts-shift{shift}"] = M.answers_over(lengths, lambda t, n: rng.permutation(np.arange(n) < want[t]))
    return vecs


def check_materialise(k, E, front, send_fp, off, answers, name):
    total = len(send_fp)
    assert len(answers) == total   # a 1 only where a candidate is: every position of the exact form holds one
    yes = answers != 0
    popcounts = [int(yes[int(off[t]):int(off[t + 1])].sum()) for t in range(k.P)]
    nblocks = sum(-(-c // 64) for c in popcounts)
    cap_states = nblocks * 64 + 64
    d_ans, d_states = device(answers), filled(cap_states * k.W)
    counts = k.eng.shard_materialise(d_ans.data_ptr(), d_states.data_ptr(), cap_states, slot=0)
    assert counts == popcounts, name
    buf = words(d_states)
    assert (buf[nblocks * 64 * k.W:] == M.FILL64).all(), name
    d_par = filled(sum(popcounts) + 8)
    k.eng.shard_materialise_parents(0, d_par.data_ptr())
    par = words(d_par)
    assert (par[sum(popcounts):] == M.FILL64).all(), name
    at = 0
    for t, (states, pad) in enumerate(M.split_blocks(buf[:nblocks * 64 * k.W], popcounts, k.W)):
        assert not pad.any(), name
        where = int(off[t]) + np.flatnonzero(yes[int(off[t]):int(off[t + 1])])
        for j, i in enumerate(where):
            state = states[j].tobytes()
            assert k.H.key(state) == E.key_of[int(send_fp[i])], (name, t, j)
            word = int(par[at + j])
            k.check_step(state, (k.r, word >> 16, word & 0xffff), front)
        at += len(where)


def check_keep(k, E, front, send_fp, answers, a_next):
    d_ans = device(answers)
    n = k.eng.shard_keep(d_ans.data_ptr(), slot=0)
    where = np.flatnonzero(answers != 0)
    assert n == len(where) and k.arena_next() == a_next + n
    for j, i in enumerate(where):
        state, *parent = k.fetch(a_next + j)
        assert k.H.key(state) == E.key_of[int(send_fp[i])], j
        k.check_step(state, parent, front)
    return a_next + n


def check_ingest(k, a_next):
    for src, n in enumerate((1, 64, 65)):
        rng = np.random.default_rng(n)
        states = rng.integers(1, 1 << 63, size=(n, k.W)).astype(np.uint64)
        idx = rng.integers(1 << 16, 1 << 32, size=n).astype(np.uint64)
        slot = rng.integers(1, 0xfff0, size=n).astype(np.uint64)
        src_rank = (k.P - 1 - src) % k.P
        d_blocks = device(M.blocked(states, k.W).view(np.int64))
        d_par = device(M.parent_word(idx, slot).view(np.int64))
        k.eng.shard_ingest(d_blocks.data_ptr(), n)
        k.eng.shard_ingest_parents(d_par.data_ptr(), n, src_rank)
        assert k.arena_next() == a_next + n
        for j in range(n):
            if k.P == 1:   # (one rank keeps no column of parent ranks: nothing arrives from elsewhere, mc_shard_ingest_parents does nothing)
                assert k.fetch(a_next + j)[:3] == (states[j].tobytes(), 0, M.NOT_LOCAL), (n, j)
                continue
            assert k.fetch(a_next + j) == (states[j].tobytes(), src_rank, int(idx[j]), int(slot[j])), (n, j)
        a_next += n
    return a_next


@pytest.mark.parametrize("name", list(R.CASES))
def test_exact_form(rank, name):
    """expand_launch + expand_finish, the locally owned new states, then materialise / materialise_parents for every crafted vector,
    keep for two, ingest + ingest_parents: no call consumes the slot's pending list (shard_materialise and shard_keep read pend_src and
    write the engine's own scratch lists), so one expand serves them all"""
    k = rank(name)
    front, E = k.frontier(), k.expected()
    check_conditions(E, k.P, k.r)
    _, send_fp, counts, off = expand_exact(k)
    check_routed(E, [send_fp[int(off[t]):int(off[t + 1])] for t in range(k.P)], counts, exact=False)
    a_next = check_local_new(k, E, front, k.n0 + k.nloc)
    if k.P > 1:
        vecs = answer_vectors(counts, 7)
        for vname, answers in vecs.items():
            check_materialise(k, E, front, send_fp, off, answers, vname)
        for vname in ("random", "last-only"):
            a_next = check_keep(k, E, front, send_fp, vecs[vname], a_next)
    else:
        assert sum(counts) == 0
    check_ingest(k, a_next)


@pytest.mark.parametrize("name", ["raft-P3-r1", "ssi-P3-r1"])
def test_routing_without_the_filter_keeps_every_candidate(rank, name):
    k = rank(name, MC_F_NOFILTER)
    E = k.expected()
    _, send_fp, counts, off = expand_exact(k)
    check_routed(E, [send_fp[int(off[t]):int(off[t + 1])] for t in range(k.P)], counts, exact=True)
    assert counts == [0 if t == k.r else n for t, n in enumerate(E.per_owner)]


# --------------------------------------------------------------------------------------------------------------------- the packed form
def expand_packed(k, cap):
    """(send_fp as P rows of cap words)"""
    send_fp = filled(k.P * cap)
    k.eng.shard_expand_launch(0, 0, k.nloc, k.P * cap)
    k.eng.shard_expand_pack(0, send_fp.data_ptr(), cap)
    return words(send_fp).reshape(k.P, cap)


@pytest.mark.parametrize("name", list(R.CASES))
def test_packed_form(rank, name):
    """expand_pack, keep_pack with answers over P * cap, end_level: the count words, the same fingerprints as the exact form, and
    kept + locally owned at the end of the level"""
    k = rank(name)
    front, E = k.frontier(), k.expected()
    cap = max([n for t, n in enumerate(E.per_owner) if t != k.r] + [1]) + 1   # room for every pair's candidate: the filter only drops
    rows = expand_packed(k, cap)
    counts = [int(rows[t, 0]) for t in range(k.P)]
    assert all(c < cap for c in counts)
    check_routed(E, [rows[t, 1:1 + counts[t]] for t in range(k.P)], counts, exact=False)
    for t in range(k.P):
        assert (rows[t, 1 + counts[t]:] == M.FILL64).all()
    a_next = check_local_new(k, E, front, k.n0 + k.nloc)
    # answers: a 1 only at a position that holds a candidate, never at a count word or behind a range's count
    rng = np.random.default_rng(11)
    answers = np.zeros((k.P, cap), dtype=np.uint8)
    for t in range(k.P):
        answers[t, 1:1 + counts[t]] = rng.random(counts[t]) < 0.5
    holds = np.zeros((k.P, cap), dtype=bool)
    for t in range(k.P):
        holds[t, 1:1 + counts[t]] = True
    assert not (answers.astype(bool) & ~holds).any()
    d_ans = device(answers.reshape(-1))
    k.eng.shard_keep_pack(0, d_ans.data_ptr(), cap)
    kept = np.flatnonzero(answers.reshape(-1))
    assert k.eng.shard_end_level() == len(kept) + len(E.local_new)
    assert k.arena_next() == a_next + len(kept)
    flat = rows.reshape(-1)
    for j, i in enumerate(kept):
        state, *parent = k.fetch(a_next + j)
        assert k.H.key(state) == E.key_of[int(flat[i])], j
        k.check_step(state, parent, front)


@pytest.mark.parametrize("name", ["raft-P3-r1", "raft-P8-r7", "ssi-P3-r1"])
def test_packed_form_refuses_a_bucket_that_is_one_short(rank, name):
    """without the filter an owner's count is the number of generating pairs: with cap one below what the largest owner needs, that
    owner's count word is 0, its range untouched, the others are as before, and the level ends with MC_EROUTE"""
    k = rank(name, MC_F_NOFILTER)
    E = k.expected()
    need = [0 if t == k.r else n + 1 for t, n in enumerate(E.per_owner)]
    cap = max(need) - 1
    rows = expand_packed(k, cap)
    refused = [t for t in range(k.P) if need[t] > cap]
    assert refused and len(refused) < k.P - 1
    for t in range(k.P):
        if t in refused:
            assert rows[t, 0] == 0 and (rows[t, 1:] == M.FILL64).all()
        else:
            n = int(rows[t, 0])
            assert n == need[t] - (t != k.r) and collections.Counter(int(f) for f in rows[t, 1:1 + n]) == collections.Counter(E.routed[t] if t != k.r else {})
    with pytest.raises(B.McError) as e:
        k.eng.shard_end_level()
    assert e.value.code == MC_EROUTE
