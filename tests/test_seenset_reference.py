"""The seen-set's reference model (tests/seenmodel.py) and graph.h's seen_find, built for the host with g++ (tests/seenshim.py:
host_find), held against each other on tables that only crafted fingerprints produce: full buckets, chains that wrap past the last bucket,
load 1.0, and a chain of exactly as many full buckets as a probe visits.  No GPU: tests/test_gpu_seenset.py runs the device code against
the same model."""
import random

import numpy as np
import pytest

import seenmodel as M
import seenshim

SLOTS = [8, 4]


def filled(nbuckets, slots, keys):
    """(the table after the keys, the model's answers)"""
    T = M.Table(nbuckets, slots)
    return T, [T.insert(k) for k in keys]


def random_keys(rng, nbuckets, slots, n, tag0=0):
    return [M.key(rng.randrange(nbuckets), rng.randrange(slots), tag0 + i, nbuckets, slots) for i in range(n)]


def check_find(T, stored, absent):
    """every stored key at the model's position, every other key (and 0) absent"""
    stored, absent = list(stored), list(absent) + [0]
    pos = seenshim.host_find(T.slots, T.nbuckets, T.words, stored + absent)
    want = [T.find(k) for k in stored] + [M.ABSENT] * len(absent)
    assert all(w != M.ABSENT for w in want[:len(stored)])
    assert pos.tolist() == want
    for k, p in zip(stored, want):
        assert int(T.words[p]) == k


# ---------------------------------------------------------------------------------------------------------------- the key builder
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("nbuckets", [1, 2, 3, 7, 1000, 2049, 4096, 12345])
def test_keys_land_where_they_are_asked_to(nbuckets, slots):
    seen = set()
    for b in sorted({0, nbuckets // 2, nbuckets - 1}):
        for j in range(slots):
            for tag in (0, 1, 77, -1):
                k = M.key(b, j, tag, nbuckets, slots)
                assert k and k not in seen
                seen.add(k)
                assert M.home(k, nbuckets) == b and M.j0_of(k, slots) == j
    # the edge words: all ones in the low half is the LAST bucket, never one beyond; zero in the low half is bucket 0
    top = M.key(nbuckets - 1, 0, -1, nbuckets, slots)
    assert top & M.M32 == M.M32 and M.home(top, nbuckets) == nbuckets - 1
    low = M.key(0, 0, 5, nbuckets, slots)
    assert low & M.M32 == 0 and low >> 32 and M.home(low, nbuckets) == 0


# ---------------------------------------------------------------------------------------------------------------- the model itself
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("nbuckets", [1, 2, 3, 5, 64])
def test_the_model_is_the_rule_word_by_word(nbuckets, slots):
    """Table.insert's shortcuts (a dictionary of the stored keys, fill counts) against the rule spelled out, past load 1.0"""
    rng = random.Random(nbuckets * 10 + slots)
    keys = random_keys(rng, nbuckets, slots, nbuckets * slots + 5)
    keys += rng.sample(keys, len(keys) // 3)
    rng.shuffle(keys)
    T, naive = M.Table(nbuckets, slots), [[0] * slots for _ in range(nbuckets)]
    for k in keys:
        assert T.insert(k) == M.insert_naive(naive, nbuckets, slots, k)
    assert T.words.tolist() == [w for b in naive for w in b]
    assert np.count_nonzero(T.words) == nbuckets * slots   # more distinct keys than slots, fewer buckets than a probe visits: full


def test_the_rotated_order():
    T, ans = filled(4, 8, [M.key(1, 6, t, 4) for t in range(10)])
    assert ans == [M.NEW] * 10
    assert [T.find(M.key(1, 6, t, 4)) for t in range(10)] == [8 + 6, 8 + 7, 8 + 0, 8 + 1, 8 + 2, 8 + 3, 8 + 4, 8 + 5, 16 + 6, 16 + 7]


# ---------------------------------------------------------------------------------------------------------------- seen_find against it
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("nbuckets", [1, 2, 3, 7, 1000, 2049])
@pytest.mark.parametrize("load", [0.5, 1.0])
def test_find_on_random_tables(nbuckets, slots, load):
    rng = random.Random(nbuckets * 100 + slots + int(load * 10))
    n = int(nbuckets * slots * load)
    keys = random_keys(rng, nbuckets, slots, n)
    T, ans = filled(nbuckets, slots, keys)
    stored = [k for k, a in zip(keys, ans) if a == M.NEW]
    assert len(stored) == n or nbuckets > M.PROBE_CAP   # (every key gets in while a probe visits every bucket)
    if load == 1.0 and nbuckets <= M.PROBE_CAP:
        assert np.count_nonzero(T.words) == nbuckets * slots
    others = random_keys(rng, nbuckets, slots, 200, tag0=n)   # the same buckets, other tags: at load 1.0 their whole sequence is full
    check_find(T, stored, others + [k for k, a in zip(keys, ans) if a == M.FULL])
    M.check_invariants(T.words, stored, nbuckets, slots)


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("nbuckets", [2, 3, 40, 1000])
def test_find_along_a_chain_that_wraps(nbuckets, slots):
    """all keys at home in the last bucket, with every j0: the chain runs on through bucket 0"""
    nkeys = min(nbuckets, 21) * slots - 3
    keys = [M.key(nbuckets - 1, t % slots, t, nbuckets, slots) for t in range(nkeys - 1)] + [M.key(nbuckets - 1, 0, -1, nbuckets, slots)]
    T, ans = filled(nbuckets, slots, keys)
    assert ans == [M.NEW] * nkeys
    assert T.find(keys[slots]) // slots == 0 and T.fill[nbuckets - 1] == slots
    check_find(T, keys, [M.key(nbuckets - 1, 1, 5000, nbuckets, slots), M.key(0, 0, 5001, nbuckets, slots)])
    M.check_invariants(T.words, keys, nbuckets, slots)


@pytest.mark.parametrize("slots", SLOTS)
def test_the_two_probe_caps_agree(slots):
    """2048 full buckets from the key's home on: the model does not store the key in the bucket behind them and seen_find does not look there"""
    nbuckets, home = 4096, 3000   # (the chain wraps: buckets 3000 .. 4095, 0 .. 951)
    chain = [M.key(home, t % slots, t, nbuckets, slots) for t in range(M.PROBE_CAP * slots)]
    T, ans = filled(nbuckets, slots, chain)
    assert ans == [M.NEW] * len(chain)
    behind = (home + M.PROBE_CAP) % nbuckets
    assert T.fill[behind] == 0 and T.fill[(behind - 1) % nbuckets] == slots
    late = M.key(home, 0, len(chain), nbuckets, slots)
    assert T.insert(late) == M.FULL
    check_find(T, chain[:50] + chain[-50:], [late])
    # had anything put it there all the same, seen_find would still answer "never stored" ...
    forced = T.words.copy()
    forced[behind * slots] = late
    assert seenshim.host_find(slots, nbuckets, forced, [late]).tolist() == [M.ABSENT]
    with pytest.raises(AssertionError, match="buckets from home"):
        M.check_invariants(forced, chain + [late], nbuckets, slots)
    # ... while a key at home one bucket further on reaches that bucket as the last of its sequence
    near = M.key(home + 1, 0, len(chain) + 1, nbuckets, slots)
    assert T.insert(near) == M.NEW and T.find(near) // slots == behind
    check_find(T, [near, chain[-1]], [late])
    M.check_invariants(T.words, chain + [near], nbuckets, slots)


# ---------------------------------------------------------------------------------------------------------------- the checker itself
@pytest.mark.parametrize("slots", SLOTS)
def test_broken_tables_are_rejected(slots):
    nbuckets = 16
    keys = [M.key(5, 1, t, nbuckets, slots) for t in range(2 * slots + 2)] + [M.key(9, 0, 100, nbuckets, slots)]
    T, _ = filled(nbuckets, slots, keys)
    M.check_invariants(T.words, keys, nbuckets, slots)
    free = int(np.nonzero(T.words == 0)[0][-1])

    dup = T.words.copy()
    dup[free] = keys[0]
    with pytest.raises(AssertionError, match="stored twice"):
        M.check_invariants(dup, keys, nbuckets, slots)

    moved = T.words.copy()   # a key of the full home bucket, one bucket on: it leaves a hole behind it
    p = T.find(keys[0])
    assert p // slots == 5 and moved[8 * slots - 1] == 0
    moved[p], moved[8 * slots - 1] = 0, keys[0]
    with pytest.raises(AssertionError, match="behind a bucket with a free slot"):
        M.check_invariants(moved, keys, nbuckets, slots)

    foreign = T.words.copy()
    foreign[free] = M.key(3, 0, 999, nbuckets, slots)
    with pytest.raises(AssertionError, match="foreign word"):
        M.check_invariants(foreign, keys, nbuckets, slots)

    gone = T.words.copy()
    gone[T.find(keys[-1])] = 0
    with pytest.raises(AssertionError, match="not stored"):
        M.check_invariants(gone, keys, nbuckets, slots)
