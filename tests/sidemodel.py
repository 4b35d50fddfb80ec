"""A reference of the side passes that run after or beside the search (DESIGN sections 14, 15, 17, 20 and 21), in plain Python over
LOGICAL rows of the table lowering (tests/_sideshim/spec_table.h), and the cases tests/test_gpu_sidepasses.py drives the kernels with.
Written from the rules, sharing no code with the kernels or with the MC_HD headers; tests/test_sidepass_reference.py holds it against
the product's host loops (tests/_sideshim/sidehost.cpp) on every case.

The rules, as the design sections state them:
  * a pair (state, slot < nslots) is GENERATED iff its status has ST_ENABLED (section 14); its action bin is action id + 1, bin 0 is
    Init's; an id whose bin lies outside [0, nbins) is counted nowhere;
  * a stored state is credited to the pair its trace record names, to Init without a parent; a record whose parent is not below the
    state cannot be one and is counted nowhere (sections 14 and 20);
  * the edge of a generated pair (section 15): a failed Assert, an evaluation error or an overflow has no successor and is dropped; a
    self loop is an edge to the state itself; otherwise the key is looked up in the seen-set: found = an edge to the state that owns the
    key; not found = dropped if the pair is out of model or breaks an invariant, else MISSING, an inconsistency.  Key 0 is nobody's.
    A stored state whose own key the seen-set does not hold is one too (first_bad = the least state << 16 | slot, slot 0xffff for the
    state itself), and so is an edge whose key no stored state owns: only the fill pass can see that one, and it meets every missing
    successor of the degree pass a second time, so its counters hold both;
  * the process of an edge is slot // maxch, the terminating disjunct's (-1) from slot ninst * maxch on (section 16); its unit is the
    table's entry for (that instance, the label it stands at in the SOURCE state), the instance's own number for a label the table
    does not hold (section 21);
  * predicate bit k of a state is set iff the predicate holds and evaluates; the least (state << 8 | k) that fails is kept (section 17);
  * -continue (section 20): see violations_model."""
import ctypes

import numpy as np

import seenmodel as SM
from sideshim import COV_MAX_BINS, FILL8, FILL16, FILL32, HEAD, VIOL_BINS, Params

EN, OOM, ASSERT, INV, SPECERR, OVERFLOW, SELF = 1, 2, 4, 8, 16, 32, 64   # mc_common.h: ST_*
NONE = 0xffffffff            # no parent; no arena index
ABSENT = SM.ABSENT
ALL = (1 << 64) - 1
BIN_DEADLOCK, BIN_FATAL = 32, 33
F_DEADLOCK = 1               # tlamc.h: MC_F_DEADLOCK
LATER = 1 << 62              # a key found while generating successors sorts behind a stored state's own
MUTANT = None                # tests/test_sidepass_reference.py: one rule of this model, deliberately wrong


def inv(k):
    return INV | (k << 8)


class State:
    """slots: (status, action id, key) triples, max_slots of them once a case is complete (those from nslots on are never to be looked at)"""

    def __init__(self, key, slots=(), nslots=None, own=0, init=EN, pred=0, fail=0, labels=()):
        self.key, self.slots, self.own, self.init, self.pred, self.fail, self.labels = key, list(slots), own, init, pred, fail, list(labels)
        self.nslots = len(self.slots) if nslots is None else nslots


class Case:
    """One input of all three drivers.  The graph is built over [0, expanded); coverage counts [lo, hi) as generated and [hi, new_hi) as
    added; the -continue passes look at the level that expanded [lo, hi) and stored [hi, new_hi)."""

    def __init__(self, states, max_slots, nbuckets, sparse, expanded=None, lo=0, hi=None, new_hi=None, chunk=256, nbins=7, ninst=3, maxch=2,
                 nlabels=4, npred=0, parent=None, pslot=None, foreign=(), seed=1):
        n = len(states)
        self.states, self.n = states, n
        self.prm = Params(max_slots, nbins, ninst, maxch)
        self.nbuckets, self.sparse, self.slots = nbuckets, sparse, (4 if sparse else 8)
        self.expanded = n if expanded is None else expanded
        self.lo, self.hi = lo, (self.expanded if hi is None else hi)
        self.new_hi = n if new_hi is None else new_hi
        self.chunk, self.nlabels, self.npred = chunk, nlabels, npred
        rng = np.random.default_rng(seed)
        self.parent = np.full(n, NONE, np.uint32) if parent is None else np.asarray(parent, np.uint32)
        self.pslot = np.zeros(n, np.uint16) if pslot is None else np.asarray(pslot, np.uint16)
        self.unit_tab = rng.permutation(100)[:max(ninst, 1) * nlabels].astype(np.int8)   # (no two entries alike)
        # the seen-set: every stored state's key, in arena order, then the keys no row owns
        t = SM.Table(nbuckets, self.slots)
        keys = [s.key for s in states]
        assert len(set(keys)) == n and 0 not in keys, "every stored state has a key of its own"
        for k in keys + list(foreign):
            assert t.insert(k) == SM.NEW
        self.table = t.words.copy()
        # slots from nslots on: enabled pairs with stored keys, which a walk that ran past nslots would count
        for s in states:
            assert s.nslots <= max_slots and len(s.slots) <= max_slots and len(s.labels) <= 8
            while len(s.slots) < max_slots:
                s.slots.append((EN, int(rng.integers(0, nbins)), keys[int(rng.integers(0, n))]))
            s.labels += [int(x) for x in rng.integers(0, nlabels + 2, size=8 - len(s.labels))]
        self.cap = sum(s.nslots for s in states[:self.expanded]) + 7

    def forget(self, key):
        """the table loses a key (its word becomes empty)"""
        at = np.flatnonzero(self.table == np.uint64(key))
        assert len(at) == 1
        self.table[at[0]] = 0

    def rows(self):
        """the rows as spec_table.h lays them out (a fresh copy each time)"""
        if getattr(self, "_rows", None) is None:
            self._rows = self._encode()
        return self._rows.copy()

    def _encode(self):
        W = HEAD + 2 * self.prm.max_slots
        r = np.zeros((self.n, W), np.uint64)
        for i, s in enumerate(self.states):
            labels = sum((lab & 0xff) << (8 * k) for k, lab in enumerate(s.labels))
            head = [s.key, s.nslots | s.own << 16 | s.init << 32, s.pred | s.fail << 32, labels]
            body = [w for st, a, f in s.slots for w in (st | (a & 0xffffffff) << 32, f)]
            r[i] = np.array(head + body, dtype=np.uint64)
        return r


# ------------------------------------------------------------------------------------------------------------------------ the seen-set
def find(words, nbuckets, slots, key):
    """the position of `key` in a finished table, by the placement rule of tests/seenmodel.py's header: the key lies in the first
    bucket of its sequence that was not full when it arrived, so a bucket with an empty word ends the walk"""
    if key == 0:
        return ABSENT
    b = SM.home(key, nbuckets)
    for _ in range(SM.PROBE_CAP):
        bucket = words[b * slots:(b + 1) * slots]
        if key in bucket:
            return b * slots + bucket.index(key)
        if 0 in bucket:
            return ABSENT
        b = (b + 1) % nbuckets
    return ABSENT


# --------------------------------------------------------------------------------------------------------------------------- the graph
def edge_kind(status, key, words, nbuckets, slots):
    """('none' | 'dropped' | 'self' | 'edge' | 'missing', position)"""
    if not status & EN:
        return "none", ABSENT
    if status & (ASSERT | SPECERR | OVERFLOW) and MUTANT != "flagged-pairs-are-looked-up":
        return "dropped", ABSENT
    if status & SELF:
        return "self", ABSENT
    pos = find(words, nbuckets, slots, key)
    if pos != ABSENT:
        return "edge", pos
    return ("dropped" if status & (OOM | INV) else "missing"), ABSENT


def graph_model(c):
    words = [int(w) for w in c.table]
    n, prm = c.n, c.prm
    slot_index = [NONE] * len(words)
    missing_states, bad = 0, ALL
    for i, s in enumerate(c.states):
        pos = find(words, c.nbuckets, c.slots, s.key)
        if pos == ABSENT:
            missing_states, bad = missing_states + 1, min(bad, i << 16 | 0xffff)
        else:
            slot_index[pos] = i
    degree, rows = [0] * (n + 1), []
    missing = dropped = 0
    for i, s in enumerate(c.states[:c.expanded]):
        row = []
        for k, (status, action, key) in enumerate(s.slots[:s.nslots]):
            kind, pos = edge_kind(status, key, words, c.nbuckets, c.slots)
            if kind == "dropped":
                dropped += 1
            elif kind == "missing":
                missing, bad = missing + 1, min(bad, i << 16 | k)
            elif kind != "none":
                row.append((k, kind, i if kind == "self" else slot_index[pos], action))
        degree[i] = len(row)
        rows.append(row)
    gc_degree = [missing_states, missing, bad, dropped, 0, max(degree)]
    offsets = np.concatenate(([0], np.cumsum(degree[:-1]))).astype(np.uint64)
    # the fill pass: what it adds to the counters, and the four columns
    dst, act = np.full(c.cap, FILL32, np.uint32), np.full(c.cap, FILL16, np.int16)
    proc, unit = np.full(c.cap, FILL8, np.int8), np.full(c.cap, FILL8, np.int8)
    at = selfs = 0
    missing *= 2
    for i, row in enumerate(rows):
        for k, kind, to, action in row:
            if to == NONE:
                missing, bad = missing + 1, min(bad, i << 16 | k)
            selfs += to == i
            p = -1 if k >= prm.ninst * prm.maxch else k // prm.maxch
            label = c.states[i].labels[p] if 0 <= p < 8 else -1
            u = -1 if p < 0 else int(c.unit_tab[p * c.nlabels + label]) if 0 <= label < c.nlabels else p
            dst[at], act[at], proc[at], unit[at] = to, action, p, u
            at += 1
    gc_fill = [missing_states, missing, bad, dropped, selfs, max(degree)]
    pred, pred_bad = np.zeros(n, np.uint32), ALL
    for i, s in enumerate(c.states if c.npred else []):
        mask = (1 << c.npred) - 1
        pred[i] = s.pred & ~s.fail & mask
        for k in range(c.npred):
            if s.fail >> k & 1:
                pred_bad = min(pred_bad, i << 8 | k)
    return dict(slot_index=np.array(slot_index, np.uint32), degree=np.array(degree, np.uint32), offsets=offsets, dst=dst, act=act, proc=proc, unit=unit,
                pred=pred, gc_degree=np.array(gc_degree, np.uint64), gc_fill=np.array(gc_fill, np.uint64), pred_bad=pred_bad, edges=at)


# ------------------------------------------------------------------------------------------------------------------------ the coverage
def coverage_model(c, base):
    """base + (generated over [lo, hi), distinct over [hi, new_hi)); also the number of records that count"""
    nb = c.prm.nbins
    bins, valid = [int(b) for b in base], 0
    for s in c.states[c.lo:c.hi]:
        for status, action, _ in s.slots[:s.nslots]:
            if status & EN and 0 <= action + 1 < nb:
                bins[action + 1] += 1
    for i in range(c.hi, c.new_hi):
        p = int(c.parent[i])
        if p == NONE:
            b = 0
        elif p < i or MUTANT == "any-record-counts":
            b = c.states[p].slots[c.pslot[i]][1] + 1
        else:
            continue
        if 0 <= b < nb:
            bins[nb + b] += 1
            valid += 1
    return np.array(bins, np.uint64), valid


# ------------------------------------------------------------------------------------------------------------------------ -continue
def viol_key(idx, slot, kind, inv_index):
    return LATER | idx << 24 | slot << 8 | inv_index << 3 | kind


def violations_model(c, stored, expanded, flags, base):
    """base + the level's passes.  Cells: column * VIOL_BINS + bin; column 0 = stored / deadlocked states (the least arena index),
    column 1 = successors outside the model and, in the fatal bin, the pairs that end the search (the least violation key).
      * a generated pair (not an overflow: that is an error of the level) with a failed Assert is fatal (kind 2), else one with an
        evaluation error is (kind 4); else one that breaks invariant k and lies outside the model counts in bin k's column 1; one that
        breaks it INSIDE the model is the stored pass's business, unless the lowering checks stored states: then a pair flags only a
        property of the step, which no stored state shows, and is fatal (kind 1) unless it is a self loop;
      * an expanded state without a generated pair is deadlocked when deadlock is checked;
      * a stored state is listed under the invariant its status names, unless the status also says Assert, evaluation error or out of
        model.  Its status is its own for a lowering that checks stored states (looked at when it is expanded: [lo, hi)); else Init's
        for a state without a parent and that of the pair its trace record names otherwise (the states the level added: [hi, new_hi);
        for Init or an unexpanded frontier: [lo, hi))."""
    bins = [int(b) for b in base]

    def note(cell, key):
        bins[cell] += 1
        bins[2 * VIOL_BINS + cell] = min(bins[2 * VIOL_BINS + cell], key)

    if expanded:
        for i in range(c.lo, c.hi):
            s, gen = c.states[i], 0
            for k, (status, _, _) in enumerate(s.slots[:s.nslots]):
                if not status & EN:
                    continue
                gen += 1
                if status & OVERFLOW:
                    continue
                which = (status >> 8) & 31
                if status & ASSERT:
                    note(VIOL_BINS + BIN_FATAL, viol_key(i, k, 2, 0))
                elif status & SPECERR:
                    note(VIOL_BINS + BIN_FATAL, viol_key(i, k, 4, 0))
                elif status & INV and status & OOM:
                    note(VIOL_BINS + which, viol_key(i, k, 1, which))
                elif status & INV and stored and not status & SELF:
                    note(VIOL_BINS + BIN_FATAL, viol_key(i, k, 1, which))
            if gen == (s.nslots if MUTANT == "deadlock-is-no-slots" else 0) and flags & F_DEADLOCK:
                note(BIN_DEADLOCK, i)
    a, b = (c.lo, c.hi) if (stored or not expanded) else (c.hi, c.new_hi)
    for i in range(a, b):
        s, p = c.states[i], int(c.parent[i])
        if stored:
            status = s.own
        elif p == NONE:
            status = s.init
        elif p < i:
            status = c.states[p].slots[c.pslot[i]][0]
        else:
            continue
        if status & INV and not status & (ASSERT | SPECERR | (0 if MUTANT == "outside-is-stored" else OOM)):
            note((status >> 8) & 31, i)
    return np.array(bins, np.uint64)


def empty_bins():
    return np.concatenate((np.zeros(2 * VIOL_BINS, np.uint64), np.full(2 * VIOL_BINS, ALL, np.uint64)))


# ------------------------------------------------------------------------------------------------------------------------------ cases
def fresh_keys(rng, count, avoid=()):
    out, seen = [], set(avoid) | {0}
    while len(out) < count:
        k = int(rng.integers(1, 1 << 63)) * 2 + int(rng.integers(0, 2))
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


# what a well-formed search leaves: an unflagged in-model successor is stored; everything else may point anywhere
def wellformed_slot(rng, keys, absent, nbins, i):
    r = int(rng.integers(0, 16))
    action = int(rng.integers(0, nbins - 1)) if nbins > 1 else 0
    there, gone = keys[int(rng.integers(0, len(keys)))], absent[int(rng.integers(0, len(absent)))]
    status, key = {
        0: (0, there), 1: (0, gone), 2: (EN | SELF, gone), 3: (EN | OOM, gone), 4: (EN | OOM | inv(int(rng.integers(0, 32))), gone),
        5: (EN | inv(int(rng.integers(0, 32))), there), 6: (EN | ASSERT, there), 7: (EN | SPECERR, gone), 8: (EN | OVERFLOW, there),
        9: (EN, keys[i]), 10: (EN | OOM, there), 11: (EN | inv(3), gone),
    }.get(r, (EN, there))
    return status, action, key


def table_for(n, sparse, k):
    """buckets for n stored states: the two small tables of the issue where they hold them, else about half full"""
    slots = 4 if sparse else 8
    small = (64, 37)[k % 2]
    return small if n + 8 <= small * slots else -(-2 * n // slots) + 5


def seeded(n, nslots_of, max_slots=40, sparse=False, k=0, chunk=256, nbins=7, lo=0, hi=None, expanded=None, npred=5, records="level", seed=0, fail_at=()):
    rng = np.random.default_rng(1000 * n + seed)
    keys = fresh_keys(rng, n)
    absent = fresh_keys(rng, 16, keys)
    states = []
    for i in range(n):
        ns = nslots_of(i, rng)
        states.append(State(keys[i], [wellformed_slot(rng, keys, absent, nbins, i) for _ in range(ns)],
                            own=int(rng.choice([0, 0, inv(int(rng.integers(0, 32))), inv(2) | OOM, inv(2) | ASSERT])),
                            init=int(rng.choice([EN, EN, EN | inv(int(rng.integers(0, 32))), EN | inv(1) | OOM])),
                            pred=int(rng.integers(0, 1 << 32)), fail=(1 << fail_at[i]) if i in fail_at else 0))
    expanded = (n - n // 5) if expanded is None else expanded
    hi = expanded if hi is None else hi
    parent, pslot = np.full(n, NONE, np.uint32), np.zeros(n, np.uint16)
    with_slots = [i for i in range(n) if states[i].nslots]
    for i in range(n):   # records: Init's states without a parent, a valid record where a parent with a slot lies below, some that cannot be one
        below = [p for p in with_slots[:64] if p < i]
        kind = int(rng.integers(0, 8))
        if records == "level" and below and kind:
            p = below[int(rng.integers(0, len(below)))]
            parent[i], pslot[i] = (p, int(rng.integers(0, states[p].nslots))) if kind > 1 else (int(rng.integers(i, n)), int(rng.integers(0, max_slots)))
    return Case(states, max_slots, table_for(n, sparse, k), sparse, expanded=expanded, lo=lo, hi=hi, chunk=chunk, nbins=nbins, npred=npred,
                parent=parent, pslot=pslot, seed=seed)


SIZES = (1, 63, 64, 65, 257, 600)
LOS = (0, 1, 63, 70, 130)


def graph_cases():
    out = {}
    for k, n in enumerate(SIZES):
        for sparse in (False, True):
            out[f"seeded-n{n}-{'sparse' if sparse else 'dense'}"] = seeded(
                n, lambda i, rng: int(rng.integers(0, 41)), sparse=sparse, k=k + sparse, chunk=(64, 128, 256)[k % 3], nbins=(2, 7, COV_MAX_BINS)[k % 3],
                expanded=n if n < 64 else None, fail_at={})
    # every lane of a wavefront at another nslots (0 .. 63 in a shuffled order per wavefront), and one state with 40 slots among empty ones
    perm = np.random.default_rng(7).permutation(64)
    out["ladder"] = seeded(130, lambda i, rng: int(perm[(i * 5) % 64]) if i < 128 else 3, max_slots=64, chunk=128, expanded=130)
    out["spike"] = seeded(257, lambda i, rng: 40 if i == 77 else 0, chunk=64, expanded=257, sparse=True, k=1)
    for lo in LOS:   # (the graph is always built from state 0: the ranges are the other drivers')
        out[f"level-lo{lo}"] = seeded(600, lambda i, rng: int(rng.integers(0, 12)), max_slots=12, lo=lo, hi=lo + 333, expanded=533, chunk=(64, 128, 256)[lo % 3],
                                      nbins=(7, 2, COV_MAX_BINS)[lo % 3], seed=lo, sparse=bool(lo & 1))
    out.update(chain_cases())
    # every instance of state i stands at label i % 3 and every edge leads to a state of another residue: a unit taken from the
    # destination's label is wrong on every edge
    rng = np.random.default_rng(9)
    keys = fresh_keys(rng, 129)
    out["labels"] = Case([State(keys[i], [(EN, j % 4, keys[(i + 1 + j % 2) % 129]) for j in range(7)], labels=[i % 3] * 8) for i in range(129)],
                         7, 37, True, chunk=64, nlabels=3, seed=9)
    out["statuses"] = status_case()
    out.update(inconsistent_cases())
    out["predicates"] = seeded(600, lambda i, rng: int(rng.integers(0, 3)), max_slots=4, npred=32, chunk=256, fail_at={5: 9, 530: 3, 531: 2}, seed=3)
    return out


def chain_cases():
    """successor keys at the end of a chain of full buckets that wraps the end of the table, in both forms and both small tables; one
    unflagged successor key is 0"""
    out = {}
    for nb, sparse in ((64, False), (37, False), (64, True), (37, True)):
        slots = 4 if sparse else 8
        # 2 * slots stored states fill the last two buckets (homes nb - 2 and nb - 1); the next states, whose keys are homed there too,
        # land in buckets 0 and 1: their lookups start at nb - 2 or nb - 1 and wrap
        keys = [SM.key(nb - 2 + (t % 2), t % slots, t, nb, slots) for t in range(2 * slots)]
        wrapped = [SM.key(nb - 2 + (t % 2), (t + 1) % slots, 100 + t, nb, slots) for t in range(slots + 3)]
        last = SM.key(nb - 1, 0, -1, nb, slots)   # low bits 0xffffffff
        plain = [SM.key(b, 1, 200 + b, nb, slots) for b in (2, 5, 9)]
        allk = keys + wrapped + [last] + plain
        states = []
        for i, key in enumerate(allk):
            sl = [(EN, i % 5, allk[(i * 7 + j * 3) % len(allk)]) for j in range(4)] + [(EN, 1, wrapped[-1]), (EN, 2, last), (EN | OOM, 3, wrapped[0])]
            states.append(State(key, sl))
        states[3].slots[1] = (EN, 4, 0)   # key 0, unflagged: nobody's
        c = Case(states, 8, nb, sparse, chunk=64, seed=nb)
        assert find([int(w) for w in c.table], nb, slots, wrapped[-1]) // slots in (0, 1, 2) and find([int(w) for w in c.table], nb, slots, last) // slots < 3
        out[f"chain-{nb}-{'sparse' if sparse else 'dense'}"] = c
    return out


def status_case():
    """every combination of the seven ST_* bits, each with a key the table holds and one it does not, under two invariant indices"""
    rng = np.random.default_rng(11)
    pairs = [(st | (which << 8), there) for st in range(128) for which, there in ((0, True), (19, False), (31, True), (7, False))]
    n = 64 + len(pairs)   # 64 expanded states with 8 pairs each, then one added state per pair: every status word is a trace record too
    keys = fresh_keys(rng, n)
    gone = fresh_keys(rng, 4, keys)
    states = [State(keys[i], own=int(rng.choice([0, inv(4), inv(31) | SPECERR])), init=int(rng.choice([EN, EN | inv(9)]))) for i in range(n)]
    parent, pslot = np.full(n, NONE, np.uint32), np.zeros(n, np.uint16)
    for j, (st, there) in enumerate(pairs):   # (a state's own key is never among its slots': that is the self-loop flag's business)
        i = j // 8
        states[i].slots.append((st, j % 6, keys[64 + j] if there else gone[j % 4]))
        states[i].nslots = len(states[i].slots)
        parent[64 + j], pslot[64 + j] = i, j % 8
    return Case(states, 8, 160, False, expanded=64, lo=0, hi=64, chunk=64, nbins=7, parent=parent, pslot=pslot, npred=3)


def inconsistent_cases():
    """a table that disagrees with the arena, three ways, each at a low and a high state index of one run (three workgroups) and once
    with the low one alone, in the last wavefront of a run"""
    out = {}
    for where, n, at in (("both", 600, (5, 590)), ("last-wavefront", 130, (129,))):
        for what in ("self", "absent", "no-index"):
            rng = np.random.default_rng(n + len(what))
            keys = fresh_keys(rng, n)
            extra = fresh_keys(rng, 4, keys)
            # (nobody's successor is one of the states at `at`: a lost state is then the only thing its loss breaks)
            states = [State(keys[i], [(EN, (i + j) % 5, keys[t + 1 if t in at else t]) for j in range(i % 4) for t in [(i * 3 + j + 1) % (n - 1)]])
                      for i in range(n)]
            for t, i in enumerate(at):
                if what == "absent":     # an in-model successor nobody stored
                    states[i].slots = [(EN, 1, keys[(i + 1) % n]), (EN, 2, extra[t]), (EN, 0, keys[(i + 2) % n])]
                elif what == "no-index":  # a successor whose key the table holds and no row owns
                    states[i].slots = [(EN, 1, keys[(i + 1) % n]), (EN, 0, keys[(i + 2) % n]), (EN, 2, extra[t])]
                states[i].nslots = len(states[i].slots)
            # (a table so empty that a forgotten key breaks nobody else's chain)
            c = Case(states, 4, n + 7, True, chunk=256, foreign=extra[:len(at)] if what == "no-index" else (), seed=n)
            if what == "self":
                for i in at:
                    c.forget(keys[i])
            out[f"inconsistent-{what}-{where}"] = c
    return out


def coverage_cases():
    out = {}
    # the lanes of a wavefront agree on the action in every slot iteration / in the even ones only
    for name, act in (("uniform", lambda i, j: j % 5), ("mixed", lambda i, j: j % 5 if j % 2 == 0 else (i * 3 + j) % 6)):
        rng = np.random.default_rng(5)
        n = 300
        keys = fresh_keys(rng, n)
        states = [State(keys[i], [(EN, act(i, j), keys[(i + j) % n]) for j in range(6)]) for i in range(n)]
        parent, pslot = np.full(n, NONE, np.uint32), np.zeros(n, np.uint16)
        for i in range(200, n):
            parent[i], pslot[i] = (i * 7) % 200, (i % 6 if name == "mixed" else 2)
        out[name] = Case(states, 6, 200, False, lo=1, hi=200, chunk=64, nbins=7, parent=parent, pslot=pslot)
    # one lane of a wavefront counts: lane 0 or lane 63 of every wavefront of both passes
    for lane in (0, 63):
        rng = np.random.default_rng(lane)
        n = 64 * 6
        keys = fresh_keys(rng, n)
        states = [State(keys[i], [(EN if i % 64 == lane else 0, j % 3, keys[j]) for j in range(3)]) for i in range(n)]
        parent, pslot = np.full(n, NONE, np.uint32), np.zeros(n, np.uint16)
        for i in range(192, n):   # the distinct pass starts at a multiple of 64: its lanes are the states' too
            parent[i], pslot[i] = (lane, 1) if i % 64 == lane else (min(i + 1, n - 1), 0)
        out[f"one-lane-{lane}"] = Case(states, 3, 100, False, lo=0, hi=192, chunk=128, nbins=7, parent=parent, pslot=pslot)
    # action ids at and beyond both ends of the bins; records without a parent, with one, and that cannot be one
    for nbins in (2, 7, COV_MAX_BINS):
        rng = np.random.default_rng(nbins)
        n = 257
        keys = fresh_keys(rng, n)
        ids = [-2, -1, 0, nbins - 2, nbins - 1, nbins, 0x7fff]
        states = [State(keys[i], [(EN, ids[(i + j) % 7], keys[(i + j) % n]) for j in range(7)]) for i in range(n)]
        parent, pslot = np.full(n, NONE, np.uint32), np.zeros(n, np.uint16)
        for i in range(130, n):
            parent[i], pslot[i] = (NONE, (i * 5) % 130, i, n - 1)[i % 4], i % 7
        out[f"ids-nbins{nbins}"] = Case(states, 7, 100, False, lo=63, hi=130, chunk=64, nbins=nbins, parent=parent, pslot=pslot)
    return out


def violation_cases():
    """name -> (case, what the test also asserts about it)"""
    out = {}
    rng = np.random.default_rng(21)
    n = 700
    keys = fresh_keys(rng, n)

    def level(slots_of, parent_of=None, own_of=None, init_of=None, lo=0, hi=600, max_slots=4, chunk=256):
        states = [State(keys[i], slots_of(i), own=own_of(i) if own_of else 0, init=init_of(i) if init_of else EN) for i in range(n)]
        parent, pslot = np.full(n, NONE, np.uint32), np.zeros(n, np.uint16)
        for i in range(n):
            if parent_of and parent_of(i) is not None:
                parent[i], pslot[i] = parent_of(i)
        return Case(states, max_slots, 400, False, expanded=hi, lo=lo, hi=hi, chunk=chunk, parent=parent, pslot=pslot)

    plain = lambda i: [(EN, 0, keys[(i + 1) % n])]   # noqa: E731
    # several invariants break within one wavefront: as pairs outside the model, as the added states' records, as the states' own status
    out["mixed-cells"] = level(lambda i: [(EN | OOM | inv(i % 5), 0, keys[i]), (EN | inv((i * 3) % 7), 1, keys[(i + 1) % n]), (EN, 2, keys[(i + 2) % n])],
                               parent_of=lambda i: ((i * 3) % 600, 1) if i >= 600 else None, own_of=lambda i: inv(i % 3) if i % 2 else 0, lo=70, chunk=128)
    # invariant 6 breaks in all three workgroups; invariant 9 only in the last one, where its minimum therefore lies
    out["three-workgroups"] = level(lambda i: [(EN | OOM | inv(6), 0, keys[i])] if i in (3, 300, 580) else [(EN | OOM | inv(9), 0, keys[i])] if i in (577, 599) else plain(i),
                                    own_of=lambda i: inv(6) if i in (9, 290, 570) else inv(9) if i in (520, 598) else 0,
                                    parent_of=lambda i: (3, 0) if i >= 690 else None)
    # (a cell's minimum always lies in the FIRST workgroup that holds one of its violators: lanes, workgroups and chunks hold rising state
    #  indices and every key rises with the index.  "The minimum in the last workgroup" is therefore shown by invariant 9 above.)
    # the only lane of its wavefront that notes anything is lane 63
    out["one-lane-63"] = level(lambda i: [(EN | OOM | inv(3), 0, keys[i])] if i % 64 == 63 else plain(i), own_of=lambda i: inv(3) if i % 64 == 63 else 0,
                               init_of=lambda i: EN | inv(3) if i % 64 == 63 else EN, lo=0, hi=333, chunk=128)
    # an Assert (and an evaluation error) at a higher index than an invariant violator of the same level
    out["assert-behind"] = level(lambda i: [(EN | OOM | inv(2), 0, keys[i])] if i == 131 else [(EN, 0, keys[1]), (EN | ASSERT | inv(5), 1, keys[2])] if i == 400 else
                                 [(EN | SPECERR, 0, keys[3])] if i == 401 else plain(i), lo=130, hi=577, chunk=64)
    # deadlocked: no slot, or every slot disabled; an overflow is generated and so is no deadlock
    out["deadlocks"] = level(lambda i: [] if i % 9 == 0 else [(0, 0, keys[1]), (0, 1, keys[2])] if i % 9 == 1 else [(EN | OVERFLOW, 0, keys[1])] if i % 9 == 2 else plain(i),
                             lo=63, hi=257)
    # Init: parentless states under their init status (and, for the lowering that checks stored states, their own)
    out["init"] = level(plain, init_of=lambda i: EN | inv(i % 4) if i % 3 == 0 else EN | inv(1) | OOM if i % 3 == 1 else EN, own_of=lambda i: inv(8) if i % 50 == 0 else 0,
                        lo=0, hi=65)
    # a pair of a lowering that checks stored states: in the model and flagged = fatal, unless it is a self loop
    out["step-property"] = level(lambda i: [(EN | inv(4), 0, keys[(i + 1) % n])] if i == 200 else [(EN | inv(4) | SELF, 0, keys[i])] if i == 100 else plain(i), lo=1, hi=333)
    out["step-property-selfloop-only"] = level(lambda i: [(EN | inv(4) | SELF, 0, keys[i])] if i == 100 else plain(i), lo=1, hi=333)
    return out


def all_cases():
    """every case of tests/test_gpu_sidepasses.py, by the name its test uses"""
    out = {f"graph/{k}": v for k, v in graph_cases().items()}
    out.update({f"coverage/{k}": v for k, v in coverage_cases().items()})
    out.update({f"violations/{k}": v for k, v in violation_cases().items()})
    return out


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = all_cases()
    return _cases


assert ctypes.sizeof(Params) == 16
