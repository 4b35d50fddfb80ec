"""What the exchange half of the sharded engine computes, in numpy, written from include/tlamc.h (mc_shard_*) and the comments of
tla_rust_amd/csrc/engine_kernels.h ("sharded step kernels"), and the cases tests/test_gpu_exchange.py drives the kernels with
(tests/test_exchange_reference.py holds both against a loop-per-element second implementation, on the CPU).

  * routing leaves nranks * NSHARD sub-buckets [owner][shard] of `subcap` entries each and one cursor per sub-bucket; a cursor beyond
    subcap means "overflowed", and what is there is the first subcap entries;
  * the exact form concatenates them owner by owner, shard by shard;
  * the packed form gives every owner `cap` words: word 0 the count, then the candidates; an owner whose candidates and count word do not
    fit, or one of whose sub-buckets overflowed, gets the count 0, nothing else written, and the level DEV_EROUTE;
  * the answers come back position for position; per owner the sources of the positively answered candidates are compacted to the start
    of the owner's range, in order;
  * states travel per owner as whole blocks of 64, word-major inside a block (word w of state j of a block at w * 64 + j), the lanes
    behind an owner's last state zero; the arena has the same layout;
  * with a moved state travels (index of its parent on the sender) << 16 | slot; a source word is slot << 24 | column of the chunk.
Nothing here knows how a kernel indexes."""
import numpy as np

NSHARD = 8
DEV_EARENA, DEV_EROUTE = 2, 8
FILL8, FILL16, FILL32, FILL64 = 0xa7, 0xa7a7, 0xa7a7a7a7, 0xa7a7a7a7a7a7a7a7
NOT_LOCAL = 0xfffffffe   # the local parent column of a state that arrived from another rank
WORLDS = (1, 2, 3, 5, 7, 8)
GRID_PASS = 64 * 256     # entries of a sub-bucket that one pass of the compaction's grid-stride loop covers


# ------------------------------------------------------------------------------------------------------------------------------- the model
def clamped(cursors, subcap):
    return np.minimum(np.asarray(cursors, dtype=np.uint64), np.uint64(subcap)).astype(np.int64)


def compact_exact(P, cursors, rt_fp, rt_src, subcap):
    """(send_fp, pend_src, the owners' counts)"""
    n = clamped(cursors, subcap)
    valid = np.arange(subcap)[None, :] < n[:, None]
    return (np.asarray(rt_fp).reshape(P * NSHARD, subcap)[valid], np.asarray(rt_src).reshape(P * NSHARD, subcap)[valid],
            n.reshape(P, NSHARD).sum(axis=1))


def compact_packed(P, cursors, rt_fp, rt_src, subcap, cap):
    """(send_fp, pend_src over P * cap pre-filled words, the error word, which owners overflowed)"""
    cursors = np.asarray(cursors, dtype=np.uint64).reshape(P, NSHARD)
    n = clamped(cursors, subcap).reshape(P, NSHARD)
    over = (cursors > np.uint64(subcap)).any(axis=1) | (n.sum(axis=1) + 1 > cap)
    fp, src = np.full((P, cap), FILL64, dtype=np.uint64), np.full((P, cap), FILL32, dtype=np.uint32)
    rt_fp, rt_src = np.asarray(rt_fp).reshape(P, NSHARD, subcap), np.asarray(rt_src).reshape(P, NSHARD, subcap)
    valid = np.arange(subcap)[None, None, :] < n[:, :, None]
    for t in range(P):
        fp[t, 0] = 0 if over[t] else n[t].sum()
        if not over[t]:
            fp[t, 1:1 + n[t].sum()] = rt_fp[t][valid[t]]
            src[t, 1:1 + n[t].sum()] = rt_src[t][valid[t]]
    return fp.reshape(-1), src.reshape(-1), (DEV_EROUTE if over.any() else 0), over


def offsets(P, lengths):
    """off[0..8]: where each owner's range starts; from P on, the total"""
    off = np.zeros(9, dtype=np.uint64)
    off[1:P + 1] = np.cumsum(np.asarray(lengths, dtype=np.uint64))
    off[P + 1:] = off[P]
    return off


def compact_new(P, answers, off, pend_src):
    """(new_src over a pre-filled buffer as long as the answers, ends[P]: the positive answers up to the end of each owner's range)"""
    yes = np.asarray(answers) != 0
    before = np.concatenate([[0], np.cumsum(yes)])
    new_src = np.full(len(yes), FILL32, dtype=np.uint32)
    ends = np.zeros(P, dtype=np.uint64)
    for t in range(P):
        lo, hi = int(off[t]), int(off[t + 1])
        kept = np.asarray(pend_src)[lo:hi][yes[lo:hi]]
        new_src[lo:lo + len(kept)] = kept
        ends[t] = before[hi]
    return new_src, ends


def counts_of(ends):
    return np.diff(np.concatenate([[0], np.asarray(ends, dtype=np.int64)]))


def parent_word(idx, slot):
    return (np.asarray(idx, dtype=np.uint64) << np.uint64(16)) | np.asarray(slot, dtype=np.uint64)


def send_parents(P, new_src, off, cnt, chunk_base):
    """owner by owner, without padding: (chunk_base + column) << 16 | slot"""
    src = np.concatenate([np.asarray(new_src, dtype=np.uint32)[int(off[t]):int(off[t]) + int(cnt[t])] for t in range(P)])
    return parent_word(np.uint64(chunk_base) + (src & np.uint32(0xffffff)).astype(np.uint64), src >> np.uint32(24))


def blocked(states, words):
    """states (n, words) -> whole blocks of 64, word-major, zero padding"""
    states = np.asarray(states, dtype=np.uint64).reshape(-1, words)
    nb = -(-len(states) // 64)
    padded = np.zeros((nb * 64, words), dtype=np.uint64)
    padded[:len(states)] = states
    return padded.reshape(nb, 64, words).transpose(0, 2, 1).reshape(-1)


def unblocked(buf, n, words):
    """the first n states of a blocked buffer, and its padding lanes"""
    nb = -(-n // 64)
    rows = np.asarray(buf, dtype=np.uint64)[:nb * 64 * words].reshape(nb, words, 64).transpose(0, 2, 1).reshape(nb * 64, words)
    return rows[:n], rows[n:]


def send_blocks(per_owner, words):
    """the state send buffer: every owner's states as whole blocks, owner by owner"""
    return np.concatenate([blocked(s, words) for s in per_owner] + [np.zeros(0, dtype=np.uint64)])


def split_blocks(buf, counts, words):
    """the inverse: per owner (states, padding lanes)"""
    out, at = [], 0
    for c in counts:
        size = -(-int(c) // 64) * 64 * words
        out.append(unblocked(buf[at:at + size], int(c), words))
        at += size
    assert at == len(buf)
    return out


def arena_words(nstates, words):
    return -(-nstates // 64) * 64 * words


def ingest(words, arena, arena_cap, arena_next, recv_blocks, n, parent):
    """(arena, parent, arena_next, the error word) after n received states were appended"""
    arena, parent = arena.copy(), parent.copy()
    rows = arena.reshape(-1, words, 64).transpose(0, 2, 1).copy().reshape(-1, words)
    states, _ = unblocked(recv_blocks, n, words)
    fits = min(n, max(arena_cap - arena_next, 0))   # a state that has no room is not written; the others are
    rows[arena_next:arena_next + fits] = states[:fits]
    parent[arena_next:arena_next + fits] = NOT_LOCAL
    arena = rows.reshape(-1, 64, words).transpose(0, 2, 1).reshape(-1)
    if arena_next + n > arena_cap:
        return arena, parent, arena_next, DEV_EARENA
    return arena, parent, arena_next + n, 0


def ingest_parents(recv_parents, src_rank, arena_next, parent, pslot, prank):
    parent, pslot, prank = parent.copy(), pslot.copy(), prank.copy()
    w = np.asarray(recv_parents, dtype=np.uint64)
    lo = arena_next - len(w)
    parent[lo:arena_next] = (w >> np.uint64(16)).astype(np.uint32)
    pslot[lo:arena_next] = (w & np.uint64(0xffff)).astype(np.uint16)
    prank[lo:arena_next] = src_rank
    return parent, pslot, prank


def gather_states(words, arena, first, count):
    """plain records, state after state"""
    rows = np.asarray(arena).reshape(-1, words, 64).transpose(0, 2, 1).reshape(-1, words)
    return rows[first:first + count].reshape(-1)


def bump(arena_next, n, arena_cap):
    return (arena_next, DEV_EARENA) if arena_next + n > arena_cap else (arena_next + n, 0)


# ------------------------------------------------------------------------------------------------------------------------------- the cases
def _distinct_u64(rng, n):
    """n different non-zero words, none of them a pre-fill: a copied entry names its origin"""
    v = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9e3779b97f4a7c15)) ^ np.uint64(rng.integers(1, 1 << 40))
    assert len(np.unique(v)) == n and FILL64 not in v
    return v


def routed(P, subcap, seed):
    """full sub-buckets: what lies behind a cursor is as distinct as what lies in front of it"""
    rng = np.random.default_rng(seed)
    n = P * NSHARD * subcap
    return _distinct_u64(rng, n), rng.permutation(n).astype(np.uint32) + np.uint32(1 << 24)


EDGES = lambda subcap: [0, 1, 63, 64, 65, 255, 256, 257, subcap - 1, subcap, subcap + 1]   # noqa: E731
HAND_SUBCAP = 600


def compact_cases():
    """name -> (P, subcap, cursors, seed)"""
    cases = {}
    for P in WORLDS:
        rng = np.random.default_rng(1000 + P)
        cur = rng.integers(0, 301, size=P * NSHARD)
        cur[rng.random(P * NSHARD) < 0.2] = 0
        cases[f"random-P{P}"] = (P, 300, cur.astype(np.uint64), 10 + P)
        edges = EDGES(HAND_SUBCAP)
        for shift in (0, 8):
            cur = np.array([edges[(b + shift) % len(edges)] for b in range(P * NSHARD)], dtype=np.uint64)
            cases[f"edges-P{P}-shift{shift}"] = (P, HAND_SUBCAP, cur, 20 + P + shift)
    # a sub-bucket longer than one pass of the grid-stride loop, another exactly full
    cur = np.array([3, GRID_PASS + 2, 0, 70, GRID_PASS + 3, 1, 0, 64] + [0, 5, GRID_PASS, 0, 0, 0, 257, 0], dtype=np.uint64)
    cases["grid-stride-P2"] = (2, GRID_PASS + 3, cur, 77)
    return cases


def packed_cap(P, cursors, subcap):
    """a capacity every owner fits: only an overflowed sub-bucket refuses"""
    return int(clamped(cursors, subcap).reshape(P, NSHARD).sum(axis=1).max()) + 6


def capacity_cases():
    """name -> (P, subcap, cursors, seed, owner, its total): the owner has strictly the most candidates"""
    cases = {}
    for P in WORLDS:
        for where, owner in {"first": 0, "middle": P // 2, "last": P - 1}.items():
            if (where == "middle" and P < 3) or (where == "last" and P < 2):
                continue
            rng = np.random.default_rng(2000 + 10 * P + owner)
            cur = rng.integers(0, 40, size=(P, NSHARD))
            cur[owner] += 40
            cur[owner, rng.integers(NSHARD)] = 0
            cases[f"P{P}-{where}"] = (P, 100, cur.reshape(-1).astype(np.uint64), 30 + P, owner, int(cur[owner].sum()))
    return cases


BLOCK_COUNTS = [0, 1, 63, 64, 65, 128, 130]
RANGE_LENGTHS = [1, 63, 64, 65, 255, 256, 257, 130]


def answers_over(lengths, fill):
    """per-range answer vectors, concatenated"""
    parts = [np.asarray(fill(t, n), dtype=np.uint8).reshape(-1) for t, n in enumerate(lengths)]
    return np.concatenate(parts + [np.zeros(0, dtype=np.uint8)])


def answer_patterns(lengths, rng):
    """name -> answers over ranges of these lengths (the vectors of the issue that any set of ranges has)"""
    def only(pos):
        def fill(t, n):
            a = np.zeros(n, dtype=np.uint8)
            if n:
                a[pos] = 1
            return a
        return fill
    pats = {
        "all-0": answers_over(lengths, lambda t, n: np.zeros(n)),
        "all-1": answers_over(lengths, lambda t, n: np.ones(n)),
        "first-only": answers_over(lengths, only(0)),
        "last-only": answers_over(lengths, only(-1)),
        "random": answers_over(lengths, lambda t, n: rng.random(n) < 0.5),
        "random-bytes": answers_over(lengths, lambda t, n: np.where(rng.random(n) < 0.5, rng.integers(1, 256, size=n), 0)),   # non-zero = keep
    }
    if len(lengths) >= 3:
        for quiet in range(1, len(lengths) - 1):
            pats[f"owner-{quiet}-all-0"] = answers_over(lengths, lambda t, n: np.zeros(n) if t == quiet else np.ones(n))
    return pats


def answer_cases():
    """name -> (P, off[9], answers, pend_src)"""
    cases = {}

    def add(name, P, lengths, answers, seed):
        total = int(np.sum(lengths))
        if total == 0:
            return
        rng = np.random.default_rng(seed)
        # a source word: slot << 24 | column, both with their high bits in use somewhere
        pend = (rng.integers(0, 256, size=total).astype(np.uint32) << np.uint32(24)) | rng.integers(0, 1 << 24, size=total).astype(np.uint32)
        assert len(answers) == total
        cases[name] = (P, offsets(P, lengths), answers, pend)

    for P in WORLDS:
        rng = np.random.default_rng(3000 + P)
        lengths = [RANGE_LENGTHS[(t + P) % len(RANGE_LENGTHS)] for t in range(P)]
        for pat, ans in answer_patterns(lengths, rng).items():
            add(f"P{P}-{pat}", P, lengths, ans, 40 + P)
        # an empty range in first, middle and last place (and two in a row)
        for where, empty in {"first": [0], "middle": [P // 2], "last": [P - 1], "two": [P // 2, P // 2 + 1]}.items():
            if (where == "middle" and P < 3) or (where == "two" and P < 5) or P < 2:
                continue
            ls = [0 if t in empty else n for t, n in enumerate(lengths)]
            for pat in ("all-1", "random", "first-only", "last-only"):
                add(f"P{P}-empty-{where}-{pat}", P, ls, answer_patterns(ls, rng)[pat], 50 + P)
        # ranges that end on multiples of 64 and of 256
        ls = [256, 64, 192, 0, 512, 256, 64, 128][:P]
        for pat in ("all-1", "random", "first-only", "last-only"):
            add(f"P{P}-aligned-{pat}", P, ls, answer_patterns(ls, rng)[pat], 55 + P)
        # the counts of the block plan: owner t keeps BLOCK_COUNTS[(t + shift) % 7] of a range that is a little longer
        for shift in range(0, len(BLOCK_COUNTS), 2 if P > 1 else 1):
            want = [BLOCK_COUNTS[(t + shift) % len(BLOCK_COUNTS)] for t in range(P)]
            ls = [c + (0 if t % 2 else 9) for t, c in enumerate(want)]
            ans = answers_over(ls, lambda t, n: rng.permutation(np.arange(n) < want[t]))
            add(f"P{P}-counts-shift{shift}", P, ls, ans, 60 + P + shift)
    return cases


def ingest_cases():
    """name -> (words, n, arena_next, arena_cap, seed)"""
    cases = {}
    for words in (1, 2, 16, 24):
        for n in (1, 63, 64, 65, 130):
            nxt = 37 if n % 2 else 100
            cases[f"w{words}-n{n}"] = (words, n, nxt, nxt + n + 29, 70 + n + words)
    cases["exact-fit"] = (2, 65, 37, 37 + 65, 91)
    cases["one-past-the-cap"] = (2, 65, 37, 37 + 65 - 1, 92)
    cases["one-past-the-cap-at-a-block-end"] = (16, 130, 62, 62 + 130 - 1, 93)
    return cases


def ingest_input(words, n, arena_next, arena_cap, seed):
    """(arena, parent, recv_blocks): a pre-filled arena, and received blocks whose padding lanes hold words that must not arrive"""
    rng = np.random.default_rng(seed)
    arena = np.full(arena_words(arena_cap, words), FILL64, dtype=np.uint64)
    parent = np.full(arena_cap, FILL32, dtype=np.uint32)
    return arena, parent, _distinct_u64(rng, arena_words(n, words))


def parent_cases():
    """name -> (recv_parents, src_rank, arena_next, columns' length)"""
    cases = {}
    for k, n in enumerate((1, 64, 65)):
        rng = np.random.default_rng(80 + n)
        idx = rng.integers(1 << 16, 1 << 32, size=n).astype(np.uint64)   # index bits above 2^16 ...
        idx[0] = 0xffff0001
        slot = rng.integers(1, 1 << 16, size=n).astype(np.uint64)        # ... and slot bits
        slot[-1] = 0xfffc
        cases[f"n{n}"] = (parent_word(idx, slot), (7, 0, 3)[k], 37 + n + 64 * k, 37 + n + 64 * k + 21)
    return cases
