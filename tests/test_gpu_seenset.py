"""The product's seen-set code (engine_kernels.h: seen_insert_t in every form, seen_insert_slow, k_probe, k_probe_packed, k_insert; graph.h:
seen_find) on crafted fingerprints and near-full tables, through the driver of tests/seenshim.py, against tests/seenmodel.py — a
sequential model of the placement rule that tests/test_seenset_reference.py holds against the rule spelled out.  Everything is exact.

  * one key at a time (a single lane): the final table equals the model's word for word, and so do the answers;
  * concurrently: for every distinct key exactly one occurrence is answered "new", seenmodel.check_invariants holds on the final table,
    and seen_find — on the device and on the host — finds every key where it lies.  Which of two equal keys wins is never looked at.

What this does NOT cover: k_expand_pairs' pipelined copy of the rule and the by-family kernel's probes (tests/test_gpu_seenset_load.py
runs them at high load through whole models), the split-phase prober (off by default) and bucket counts near 2^32."""
import functools
import random

import numpy as np
import pytest

import seenmodel as M
import seenshim as S
from testlib import build_mutants, mutant_tree, survives

pytestmark = pytest.mark.gpu

THIN = [S.PLAIN, S.BLIND, S.PRE]
SERIAL_FORMS = [(slots, form) for slots in (8, 4) for form in THIN + [S.SLOW]]
CONCURRENT_FORMS = [(slots, form) for slots in (8, 4) for form in THIN + [S.SLOW, S.KPROBE]]


def form_id(sf):
    return f"{sf[0]}-{S.FORM_NAMES[sf[1]]}"


# ---------------------------------------------------------------------------------------------------------------- one at a time
def compare_serial(slots, form, nbuckets, keys, start=None, L=None):
    """keys, in order, by one lane into the table `start` (a seenmodel.Table; default: empty): answers, error bits and every word of the final
    table are the model's.  Then all of them once more, concurrently: all known, the table unchanged.  Returns the model's table and answers."""
    T = start.copy() if start else M.Table(nbuckets, slots)
    table = T.words.copy()
    want = [T.insert(k) for k in keys]
    ans, errs, _ = S.insert_keys(form, slots, nbuckets, table, keys, serial=True, L=L)
    assert ans.tolist() == [w == M.NEW for w in want]
    assert errs.tolist() == [S.DEV_ETABLE if w == M.FULL else 0 for w in want]
    assert np.array_equal(table, T.words)
    stored = [k for k, w in zip(keys, want) if w != M.FULL]
    ans, errs, _ = S.insert_keys(form, slots, nbuckets, table, stored, L=L)
    assert not ans.any() and not errs.any()
    assert np.array_equal(table, T.words)
    return T, want


def random_keys(rng, nbuckets, slots, n, tag0=0):
    return [M.key(rng.randrange(nbuckets), rng.randrange(slots), tag0 + i, nbuckets, slots) for i in range(n)]


@pytest.mark.parametrize("sf", SERIAL_FORMS, ids=form_id)
def test_one_home_bucket_and_one_j0(sf):
    slots, form = sf
    T, want = compare_serial(slots, form, 1000, [M.key(500, 3, t, 1000, slots) for t in range(30 * slots + 1)])
    assert want == [M.NEW] * len(want) and T.fill[500:530].tolist() == [slots] * 30 and T.fill[530] == 1


@pytest.mark.parametrize("sf", SERIAL_FORMS, ids=form_id)
@pytest.mark.parametrize("nbuckets", [2, 1000])
def test_a_chain_from_the_last_bucket_wraps_to_bucket_0(sf, nbuckets):
    """... with every j0, and the largest low half there is (0xffffffff: the last bucket, not one beyond the table)"""
    slots, form = sf
    n = min(nbuckets, 12) * slots - 2
    keys = [M.key(nbuckets - 1, 0, -1, nbuckets, slots)] + [M.key(nbuckets - 1, t % slots, t, nbuckets, slots) for t in range(n - 1)]
    T, want = compare_serial(slots, form, nbuckets, keys)
    assert want == [M.NEW] * n and T.fill[nbuckets - 1] == slots and T.fill[0] > 0


@pytest.mark.parametrize("sf", SERIAL_FORMS, ids=form_id)
def test_the_one_free_slot_is_the_last_in_the_keys_order(sf):
    """bucket i + 1 is left with slot i free; a key whose order starts right behind it gets there after trying every other slot"""
    slots, form = sf
    nbuckets, start, late = slots + 2, M.Table(slots + 2, slots), []
    for i in range(slots):
        for r in range(1, slots):
            assert start.insert(M.key(i + 1, (i + r) % slots, r, nbuckets, slots)) == M.NEW   # each takes the slot its order starts at
        late.append(M.key(i + 1, (i + 1) % slots, 100 + i, nbuckets, slots))
    T, want = compare_serial(slots, form, nbuckets, late, start=start)
    assert want == [M.NEW] * slots and [T.find(k) for k in late] == [(i + 1) * slots + i for i in range(slots)]


@pytest.mark.parametrize("sf", SERIAL_FORMS, ids=form_id)
@pytest.mark.parametrize("nbuckets", [1, 2, 3, 1000])
def test_load_one_and_one_key_more(sf, nbuckets):
    """fewer buckets than a probe visits: every key gets in while there is a free slot, and the first key after that raises DEV_ETABLE"""
    slots, form = sf
    rng = random.Random(nbuckets * 10 + slots)
    keys = random_keys(rng, nbuckets, slots, nbuckets * slots + 1)
    T, want = compare_serial(slots, form, nbuckets, keys + keys[:3])
    assert want == [M.NEW] * (nbuckets * slots) + [M.FULL] + [M.KNOWN] * 3
    assert np.count_nonzero(T.words) == nbuckets * slots


@pytest.mark.parametrize("sf", SERIAL_FORMS, ids=form_id)
def test_load_one_with_more_buckets_than_a_probe_visits(sf):
    slots, form = sf
    nbuckets = M.PROBE_CAP + 1
    keys = random_keys(random.Random(slots), nbuckets, slots, nbuckets * slots)
    T, want = compare_serial(slots, form, nbuckets, keys)
    assert want.count(M.NEW) >= nbuckets * slots - 1   # (the last free slot may lie in the one bucket a key's sequence leaves out)


@functools.lru_cache(maxsize=None)
def chain_from_bucket_0(slots, nbuckets=4096):
    """(as many keys at home in bucket 0 as 2048 buckets hold, the model's table after all but the last two buckets of them; computed once,
    copied by compare_serial)"""
    chain = [M.key(0, t % slots, t, nbuckets, slots) for t in range(M.PROBE_CAP * slots)]
    start = M.Table(nbuckets, slots)
    for k in chain[:-2 * slots]:
        assert start.insert(k) == M.NEW
    return chain, start


@pytest.mark.parametrize("sf", SERIAL_FORMS, ids=form_id)
def test_the_probe_cap(sf):
    """4096 buckets, 2048 of them filled from bucket 0 on by keys at home there: the keys that still arrive for bucket 0 raise DEV_ETABLE —
    and the call returns.  (The chain's first 2046 buckets are the model's; the device fills the last two.)"""
    slots, form = sf
    nbuckets, extra = 4096, 3
    chain, start = chain_from_bucket_0(slots)
    more = [M.key(0, t % slots, len(chain) + t, nbuckets, slots) for t in range(extra)]
    keys = chain[-2 * slots:] + more[:1] + chain[:2] + more[1:] + [M.key(1, 0, 9999999, nbuckets, slots)]
    T, want = compare_serial(slots, form, nbuckets, keys, start=start)
    assert want.count(M.FULL) == extra and want[-1] == M.NEW and T.find(keys[-1]) // slots == M.PROBE_CAP
    assert T.fill[:M.PROBE_CAP].tolist() == [slots] * M.PROBE_CAP


@pytest.mark.parametrize("sf", CONCURRENT_FORMS, ids=form_id)
def test_the_probe_cap_with_every_key_in_flight(sf):
    """the same chain in one launch, from an empty table: whichever keys come last, exactly `extra` of them find 2048 full buckets"""
    slots, form = sf
    nbuckets, extra = 4096, 5
    keys = np.array(chain_from_bucket_0(slots)[0] + [M.key(0, t % slots, M.PROBE_CAP * slots + t, nbuckets, slots) for t in range(extra)], dtype=np.uint64)
    table = S.empty_table(nbuckets, slots)
    ans, errs, cerr = S.insert_keys(form, slots, nbuckets, table, keys)
    if form == S.KPROBE:
        assert cerr == S.DEV_ETABLE
    else:
        assert set(np.unique(errs).tolist()) == {0, S.DEV_ETABLE} and np.array_equal(errs != 0, ~ans)
    assert np.count_nonzero(~ans) == extra
    M.check_invariants(table, keys[ans].tolist(), nbuckets, slots)
    assert not table[M.PROBE_CAP * slots:].any()


def test_k_probe_one_launch_per_key():
    for slots in (8, 4):
        keys = random_keys(random.Random(7), 3, slots, 3 * slots + 1)
        T, table = M.Table(3, slots), S.empty_table(3, slots)
        want = [T.insert(k) for k in keys + keys[:3]]
        ans, _, cerr = S.insert_keys(S.KPROBE, slots, 3, table, keys + keys[:3], serial=True)
        assert ans.tolist() == [w == M.NEW for w in want] and want.count(M.FULL) == 1
        assert cerr == S.DEV_ETABLE and np.array_equal(table, T.words)


# ---------------------------------------------------------------------------------------------------------------- concurrently
def check_concurrent(slots, form, nbuckets, keys, table=None, known=(), L=None):
    """one launch over `keys` (with repeats) into `table`, which holds `known`: the answers, the final table and both seen_find's.
    No key may meet a full table here.  Returns the table."""
    table = S.empty_table(nbuckets, slots) if table is None else table
    keys = np.asarray(keys, dtype=np.uint64)
    ans, errs, cerr = S.insert_keys(form, slots, nbuckets, table, keys, L=L)
    assert not errs.any() and cerr == 0
    distinct, inv = np.unique(keys, return_inverse=True)
    news = np.bincount(inv, weights=ans, minlength=len(distinct)).astype(np.int64)
    was_known = np.isin(distinct, np.fromiter(known, dtype=np.uint64, count=len(known)))
    assert np.array_equal(news, np.where(was_known, 0, 1)), "not exactly one occurrence of every new key (and none of a known one) is answered new"
    everything = set(distinct.tolist()) | set(known)
    where = M.check_invariants(table, everything, nbuckets, slots)
    probe = sorted(everything)
    absent = [M.key(b % nbuckets, b % slots, (1 << 27) + b, nbuckets, slots) for b in range(40)] + [0]
    want = [where[k] for k in probe] + [M.ABSENT] * len(absent)
    assert S.find(slots, nbuckets, table, probe + absent, L=L).tolist() == want
    assert S.host_find(slots, nbuckets, table, probe + absent).tolist() == want
    return table


def with_repeats(keys):
    """about a third of the occurrences repeat an earlier key: the next lane, the next wavefront, the next workgroup"""
    keys = list(keys)
    for n, i in enumerate(range(0, len(keys), 3)):
        off = (1, 64, 256)[n % 3]
        if i + off < len(keys):
            keys[i + off] = keys[i]
    return keys


def buckets_for(ndistinct, slots, load=0.9):
    return max(1, -(-ndistinct // int(slots * load)))


@pytest.mark.parametrize("sf", CONCURRENT_FORMS, ids=form_id)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_concurrent_inserts(sf, n):
    slots, form = sf
    nbuckets = buckets_for(n, slots)
    keys = with_repeats(random_keys(random.Random(n + slots), nbuckets, slots, n))
    assert n < 257 or len(set(keys)) < 0.85 * n
    check_concurrent(slots, form, nbuckets, keys)


@pytest.mark.parametrize("sf", CONCURRENT_FORMS, ids=form_id)
def test_a_wavefront_of_one_key(sf):
    slots, form = sf
    k = M.key(2, 1, 0, 5, slots)
    check_concurrent(slots, form, 5, [k] * 64)
    check_concurrent(slots, form, 5, [M.key(4, 0, -1, 5, slots)] * 64 + [k] * 256 + [M.key(0, 0, 1, 5, slots)] * 64)


def one_home_slot(slots, nbuckets=40):
    return [M.key(nbuckets - 3, 2, t, nbuckets, slots) for t in range(64)]


@pytest.mark.parametrize("sf", CONCURRENT_FORMS, ids=form_id)
def test_a_wavefront_of_keys_for_one_home_slot(sf):
    """64 different keys, one home bucket, one j0: 63 lose the first compare-and-swap, and the chain they build wraps"""
    slots, form = sf
    check_concurrent(slots, form, 40, one_home_slot(slots))


@pytest.mark.parametrize("sf", CONCURRENT_FORMS, ids=form_id)
@pytest.mark.parametrize("load", [0.5, 0.9, 1.0])
def test_a_random_mix(sf, load):
    slots, form = sf
    nbuckets = 4096 // slots
    ndistinct = int(4096 * load)
    rng = random.Random(int(load * 10) + slots)
    keys = random_keys(rng, nbuckets, slots, ndistinct)
    keys += rng.choices(keys, k=ndistinct // 2)   # a third of the occurrences are repeats
    rng.shuffle(keys)
    table = check_concurrent(slots, form, nbuckets, keys)
    assert np.count_nonzero(table) == ndistinct   # the load the test is about


@pytest.mark.parametrize("sf", CONCURRENT_FORMS, ids=form_id)
def test_a_second_launch_into_the_same_table(sf):
    """what consecutive chunks of a level do: known and new keys mixed"""
    slots, form = sf
    nbuckets = 300
    rng = random.Random(slots)
    first = with_repeats(random_keys(rng, nbuckets, slots, 150 * slots))
    table = check_concurrent(slots, form, nbuckets, first)
    second = with_repeats(random_keys(rng, nbuckets, slots, 120 * slots, tag0=len(first))) + rng.sample(sorted(set(first)), 60 * slots)
    rng.shuffle(second)
    before = table.copy()
    check_concurrent(slots, form, nbuckets, second, table=table, known=set(first))
    assert np.array_equal(table[before != 0], before[before != 0])   # entries are write-once


# ---------------------------------------------------------------------------------------------------------------- k_probe_packed
COUNTS = lambda cap: [cap - 1, cap, 0, 17, 1 << 40, 256, 255, 1]   # (cap and more cannot be: such a bucket counts as empty)


@pytest.mark.parametrize("slots", [8, 4])
@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
def test_k_probe_packed(slots, nranks):
    cap = 300   # not a multiple of the workgroup: two workgroups per rank, the second with 44 entries
    rng = random.Random(nranks * 10 + slots)
    counts = COUNTS(cap)[:nranks]
    nbuckets = buckets_for(cap * nranks, slots)
    pool = random_keys(rng, nbuckets, slots, cap * nranks // 2)   # (ranks send each other's keys, and their own twice)
    traps = iter(random_keys(rng, nbuckets, slots, cap * nranks, tag0=1 << 20))
    fps, live = np.zeros(cap * nranks, dtype=np.uint64), np.zeros(cap * nranks, dtype=bool)
    for s, c in enumerate(counts):
        fps[s * cap] = c
        n = c if c < cap else 0
        for j in range(1, cap):
            live[s * cap + j] = j <= n
            fps[s * cap + j] = rng.choice(pool) if j <= n else next(traps)   # beyond the count: keys that must not get in
    table = S.empty_table(nbuckets, slots)
    ans, cerr = S.probe_packed(slots, nbuckets, table, fps, cap, nranks)
    assert cerr == 0
    assert set(np.unique(ans).tolist()) <= {0, 1}, "an entry was not answered"
    assert not ans[~live].any()
    distinct, inv = np.unique(fps[live], return_inverse=True)
    assert np.array_equal(np.bincount(inv, weights=ans[live], minlength=len(distinct)).astype(np.int64), np.ones(len(distinct), dtype=np.int64))
    M.check_invariants(table, distinct.tolist(), nbuckets, slots)   # (a trap or a count word in the table is a foreign word)


# ---------------------------------------------------------------------------------------------------------------- k_insert
SENTINEL = 0xdeadbeef


@pytest.mark.parametrize("slots", [8, 4])
@pytest.mark.parametrize("ncols", [1, 150, 333])
def test_k_insert(slots, ncols):
    """the matrix form: ncols no multiple of 64, nsl per column from 0 on, rows at and beyond max_slots ignored, 0 = no candidate"""
    grid_y, max_slots, row_stride = 6, 4, ncols + 11
    rng = random.Random(ncols + slots)
    nbuckets = buckets_for(ncols * max_slots + 40, slots)
    known = random_keys(rng, nbuckets, slots, 40)
    T = M.Table(nbuckets, slots)
    assert all(T.insert(k) == M.NEW for k in known)
    pool = random_keys(rng, nbuckets, slots, ncols * 2, tag0=1000) + known
    traps = iter(random_keys(rng, nbuckets, slots, grid_y * row_stride, tag0=1 << 20))
    nsl = np.array([rng.choice([0, 1, 3, 4, 6]) for _ in range(ncols)], dtype=np.uint16)
    nsl[0] = 0 if ncols > 1 else 6
    cand, live = np.zeros((grid_y, row_stride), dtype=np.uint64), {}
    for slot in range(grid_y):
        for col in range(row_stride):
            if col < ncols and slot < min(int(nsl[col]), max_slots):
                fp = 0 if rng.random() < 0.2 else rng.choice(pool)
                cand[slot, col] = fp
                if fp:
                    live[(col, slot)] = fp
            else:
                cand[slot, col] = next(traps)   # what the kernel must not look at
    table, newlist = T.words.copy(), np.full(ncols * max_slots + 7, SENTINEL, dtype=np.uint32)
    n_new, cells, err = S.k_insert(slots, nbuckets, table, cand, ncols, nsl, max_slots, newlist)
    new_keys = set(live.values()) - set(known)
    assert err == 0
    assert cells == len(live)
    assert n_new == len(new_keys)
    entries = [(int(e) & 0xffffff, int(e) >> 24) for e in newlist[:n_new]]
    assert all(e in live for e in entries)
    assert sorted(live[e] for e in entries) == sorted(new_keys)   # one entry per new key, whichever of its occurrences
    assert (newlist[n_new:] == SENTINEL).all()
    M.check_invariants(table, new_keys | set(known), nbuckets, slots)


# ---------------------------------------------------------------------------------------------------------------- mutants of the device code
# Three edits of engine_kernels.h, each of which changes a compared value, a returned flag or the choice among the slots of one bucket
# (masked to the bucket) and never an address computation, the wrap, a bucket index or a loop bound: every mutant stays inside the table
# and ends.
#   * the bucket comparison misses slot 0: a known key that lies there is answered "new" and stored a second time.  Caught by
#     compare_serial (the answers and the table of the second, all-known pass) in test_the_comparison_misses_a_slot;
#   * after a lost compare-and-swap the bucket's other free slots are abandoned: a hole behind a key.  Caught by check_invariants
#     ("behind a bucket with a free slot") in the case of 64 keys for one home slot;
#   * j0 from bits 33..: a placement that satisfies every invariant and disagrees with the rule the pipelined prober and the model
#     follow.  Caught word for word by compare_serial in the chain with every j0.
MUTANTS = {
    "compare-misses-slot-0": ("hit |= slot[i] == fp;", "hit |= i != 0 && slot[i] == fp;"),
    "lost-cas-leaves-the-bucket": ("rot &= rot - 1;", "rot = 0;"),
    "j0-from-other-bits": ("const unsigned j0 = (unsigned)(fp >> 32) & (unsigned)(SLOTS - 1);", "const unsigned j0 = (unsigned)(fp >> 33) & (unsigned)(SLOTS - 1);"),
}


@functools.lru_cache(maxsize=None)
def mutant_libraries():
    top = S.SHIM_DIR / "_build" / "mutants"   # (kept between runs: an unchanged mutant stays fresh)
    return build_mutants(MUTANTS, lambda name: S.build(csrc=mutant_tree(top, name, ("engine_kernels.h", *MUTANTS[name])), out=top / name))


@pytest.fixture(scope="module")
def mutants():
    return {name: S.load(so) for name, so in mutant_libraries().items()}


def test_the_comparison_misses_a_slot(mutants):
    keys = [M.key(b, j, b * 8 + j, 6, 8) for b in range(6) for j in range(8)][:40]

    def compare(L=None):
        compare_serial(8, S.PLAIN, 6, keys, L=L)
    assert not survives(lambda: compare(mutants["compare-misses-slot-0"]))
    compare()


def test_abandoned_free_slots_are_caught(mutants):
    def compare(L=None):
        check_concurrent(8, S.PLAIN, 40, one_home_slot(8), L=L)
    assert not survives(lambda: compare(mutants["lost-cas-leaves-the-bucket"]))
    compare()


def test_another_j0_is_caught(mutants):
    keys = [M.key(9, t % 8, t, 10, 8) for t in range(30)]

    def compare(L=None):
        compare_serial(8, S.PLAIN, 10, keys, L=L)
    assert not survives(lambda: compare(mutants["j0-from-other-bits"]))
    compare()
