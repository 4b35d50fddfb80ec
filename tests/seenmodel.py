"""A sequential model of the seen-set's placement rule (engine_kernels.h: seen_insert_t; graph.h: seen_find_t), in plain Python / numpy and
sharing no code with either:

  * the home bucket of a fingerprint is ((fp & 0xffffffff) * nbuckets) >> 32;
  * inside a bucket the slots are tried in rotated order, from j0 = (fp >> 32) & (SLOTS - 1);
  * a key goes to the first bucket of home, home + 1, ... (wrapping to bucket 0) that is not full, unless a bucket on the way holds it;
  * after PROBE_CAP buckets the table counts as full.

Inserted one key at a time the final table is fully determined (Table.words: compare word for word); for concurrent inserts
check_invariants says what must hold whatever the interleaving was."""
import numpy as np

PROBE_CAP = 2048
NEW, KNOWN, FULL = "new", "known", "full"
ABSENT = 0xffffffffffffffff   # graph.h: GRAPH_ABSENT
M32 = 0xffffffff


def home(fp, nbuckets):
    return ((fp & M32) * nbuckets) >> 32


def j0_of(fp, slots):
    return (fp >> 32) & (slots - 1)


def key(bucket, j0, tag, nbuckets, slots=8):
    """a non-zero fingerprint with home bucket `bucket` and rotated start `j0`, distinct per tag (tag >= 0; below 2^28).  The low 32 bits
    are the smallest that land in the bucket, so bucket 0 gets low bits 0 (the key is non-zero by its high bits); tag -1 asks for the
    LARGEST low bits of the bucket instead: 0xffffffff for bucket nbuckets - 1."""
    assert 0 <= bucket < nbuckets and 0 <= j0 < slots and -1 <= tag < (1 << 28)
    shift = 32 + slots.bit_length() - 1   # the tag lives above the bits of j0
    if tag == -1:
        lo = (((bucket + 1) << 32) + nbuckets - 1) // nbuckets - 1
        hi = (1 << 28) << (shift - 32)
    else:
        lo = ((bucket << 32) + nbuckets - 1) // nbuckets
        hi = (tag + 1) << (shift - 32)
    fp = ((hi | j0) << 32) | lo
    assert fp and fp < (1 << 64) and home(fp, nbuckets) == bucket and j0_of(fp, slots) == j0
    return fp


class Table:
    """nbuckets x slots words; 0 = empty"""

    def __init__(self, nbuckets, slots):
        assert slots in (4, 8) and nbuckets >= 1
        self.nbuckets, self.slots = nbuckets, slots
        self.t = np.zeros((nbuckets, slots), dtype=np.uint64)
        self.fill = np.zeros(nbuckets, dtype=np.int64)
        self.pos = {}   # key -> position (bucket * slots + slot)

    @property
    def words(self):
        return self.t.reshape(-1)

    def copy(self):
        c = Table(self.nbuckets, self.slots)
        c.t, c.fill, c.pos = self.t.copy(), self.fill.copy(), dict(self.pos)
        return c

    def _first_not_full(self, bk):
        """the first bucket of the probe sequence from bk that has a free slot, or None within PROBE_CAP buckets"""
        n = self.nbuckets
        span = min(PROBE_CAP, n)   # (a sequence longer than the table only meets the same buckets again)
        seq = (bk + np.arange(span)) % n
        free = np.nonzero(self.fill[seq] < self.slots)[0]
        return int(seq[free[0]]) if len(free) else None

    def insert(self, fp):
        """new / known / full.  A stored key is always met before a free slot: no bucket before it was ever anything but full."""
        assert 0 < fp < (1 << 64)
        if fp in self.pos:
            return KNOWN
        b = self._first_not_full(home(fp, self.nbuckets))
        if b is None:
            return FULL
        j = j0_of(fp, self.slots)
        for r in range(self.slots):
            i = (j + r) & (self.slots - 1)
            if self.t[b, i] == 0:
                self.t[b, i] = fp
                self.fill[b] += 1
                self.pos[fp] = b * self.slots + i
                return NEW
        raise AssertionError("a bucket that is not full has a free slot")

    def find(self, fp):
        return self.pos.get(fp, ABSENT)


def insert_naive(t, nbuckets, slots, fp):
    """the rule once more, bucket by bucket and word by word over a list of lists: what Table.insert's shortcuts are held against"""
    bk = home(fp, nbuckets)
    for _ in range(PROBE_CAP):
        if fp in t[bk]:
            return KNOWN
        for r in range(slots):
            i = (j0_of(fp, slots) + r) % slots
            if t[bk][i] == 0:
                t[bk][i] = fp
                return NEW
        bk = 0 if bk + 1 == nbuckets else bk + 1
    return FULL


def check_invariants(table, keys, nbuckets, slots):
    """What holds after ANY interleaving of concurrent inserts of `keys` (the distinct keys that were inserted and not answered "full"):
    each occurs exactly once and nothing else does; each sits in a bucket of its own probe sequence, fewer than PROBE_CAP buckets from
    home; every bucket of the sequence before it is completely full (what seen_find relies on).  Raises AssertionError."""
    t = np.asarray(table, dtype=np.uint64).reshape(nbuckets, slots)
    keys = {int(k) for k in keys}
    assert 0 not in keys
    flat = t.reshape(-1)
    at = np.nonzero(flat)[0]
    stored = [int(w) for w in flat[at]]
    where = {}
    for p, w in zip(at.tolist(), stored):
        assert w in keys, f"a foreign word {w:#x} at position {p}"
        assert w not in where, f"key {w:#x} is stored twice, at positions {where[w]} and {p}"
        where[w] = p
    missing = keys - set(where)
    assert not missing, f"{len(missing)} keys are not stored, such as {min(missing):#x}"
    full = np.all(t != 0, axis=1).astype(np.int64)
    run = np.concatenate(([0], np.cumsum(np.concatenate((full, full)))))   # full buckets before index i of the table laid out twice
    for k, p in where.items():
        h, b = home(k, nbuckets), p // slots
        dist = (b - h) % nbuckets
        assert dist < PROBE_CAP, f"key {k:#x} lies {dist} buckets from home"
        assert run[h + dist] - run[h] == dist, f"key {k:#x} (home {h}) lies in bucket {b} behind a bucket with a free slot"
    return where
