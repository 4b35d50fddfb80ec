"""tests/xchgmodel.py against a second implementation that walks element by element, on the cases tests/test_gpu_exchange.py drives
the kernels with, and the conditions those cases rely on: a GPU test cannot pass because its input was degenerate.  No GPU."""
import numpy as np
import pytest

import xchgmodel as M

NS = M.NSHARD


# ------------------------------------------------------------------------------------------------------------- one element at a time
def naive_compact_exact(P, cursors, rt_fp, rt_src, subcap):
    fp, src, counts = [], [], [0] * P
    for owner in range(P):
        for shard in range(NS):
            b = owner * NS + shard
            for j in range(min(int(cursors[b]), subcap)):
                fp.append(int(rt_fp[b * subcap + j]))
                src.append(int(rt_src[b * subcap + j]))
                counts[owner] += 1
    return fp, src, counts


def naive_compact_packed(P, cursors, rt_fp, rt_src, subcap, cap):
    fp, src, err, over = [M.FILL64] * (P * cap), [M.FILL32] * (P * cap), 0, []
    for owner in range(P):
        mine, spilt = [], False
        for shard in range(NS):
            b = owner * NS + shard
            spilt = spilt or int(cursors[b]) > subcap
            for j in range(min(int(cursors[b]), subcap)):
                mine.append((int(rt_fp[b * subcap + j]), int(rt_src[b * subcap + j])))
        refused = spilt or len(mine) + 1 > cap
        over.append(refused)
        if refused:
            fp[owner * cap], err = 0, M.DEV_EROUTE
            continue
        fp[owner * cap] = len(mine)
        for k, (f, s) in enumerate(mine):
            fp[owner * cap + 1 + k], src[owner * cap + 1 + k] = f, s
    return fp, src, err, over


def naive_compact_new(P, answers, off, pend_src):
    new_src, ends, seen = [M.FILL32] * len(answers), [], 0
    for t in range(P):
        k = 0
        for i in range(int(off[t]), int(off[t + 1])):
            if answers[i]:
                new_src[int(off[t]) + k] = int(pend_src[i])
                k += 1
        seen += k
        ends.append(seen)
    return new_src, ends


def naive_send_parents(P, new_src, off, cnt, chunk_base):
    out = []
    for t in range(P):
        for k in range(int(cnt[t])):
            s = int(new_src[int(off[t]) + k])
            out.append(((chunk_base + (s % (1 << 24))) * 65536) + s // (1 << 24))
    return out


def naive_blocked(states, words):
    out = [0] * (-(-len(states) // 64) * 64 * words)
    for j, st in enumerate(states):
        for w in range(words):
            out[(j // 64) * words * 64 + w * 64 + j % 64] = int(st[w])
    return out


def naive_arena_get(arena, words, idx):
    return [int(arena[(idx // 64) * words * 64 + w * 64 + idx % 64]) for w in range(words)]


# ------------------------------------------------------------------------------------------------------------------------ the compaction
COMPACT = M.compact_cases()


@pytest.mark.parametrize("name", [n for n in COMPACT if not n.startswith("grid")])
def test_compaction_model(name):
    P, subcap, cursors, seed = COMPACT[name]
    rt_fp, rt_src = M.routed(P, subcap, seed)
    fp, src, counts = M.compact_exact(P, cursors, rt_fp, rt_src, subcap)
    nfp, nsrc, ncounts = naive_compact_exact(P, cursors, rt_fp, rt_src, subcap)
    assert fp.tolist() == nfp and src.tolist() == nsrc and counts.tolist() == ncounts
    cap = M.packed_cap(P, cursors, subcap)
    pfp, psrc, err, over = M.compact_packed(P, cursors, rt_fp, rt_src, subcap, cap)
    nfp, nsrc, nerr, nover = naive_compact_packed(P, cursors, rt_fp, rt_src, subcap, cap)
    assert pfp.tolist() == nfp and psrc.tolist() == nsrc and err == nerr and over.tolist() == nover
    # at this capacity an owner is refused exactly when one of its sub-buckets ran over
    assert over.tolist() == (np.asarray(cursors).reshape(P, NS) > subcap).any(axis=1).tolist()


def test_the_grid_stride_case_needs_a_second_pass():
    P, subcap, cursors, seed = COMPACT["grid-stride-P2"]
    assert subcap > M.GRID_PASS and (cursors > M.GRID_PASS).any() and (cursors == M.GRID_PASS).any() and cursors.max() == subcap
    assert all(s <= 600 for n, (_, s, _, _) in COMPACT.items() if n != "grid-stride-P2")
    rt_fp, rt_src = M.routed(P, subcap, seed)
    fp, src, counts = M.compact_exact(P, cursors, rt_fp, rt_src, subcap)
    assert counts.tolist() == [int(cursors[:8].sum()), int(cursors[8:].sum())]
    at = 0   # (a million-element loop is too slow here: bucket by bucket)
    for b in range(P * NS):
        n = int(cursors[b])
        assert (fp[at:at + n] == rt_fp[b * subcap:b * subcap + n]).all() and (src[at:at + n] == rt_src[b * subcap:b * subcap + n]).all()
        at += n
    assert at == len(fp)


def test_the_hand_made_cursors_hold_every_edge():
    for P in M.WORLDS:
        found, refused, kept = set(), False, False
        for shift in (0, 8):
            _, subcap, cursors, _ = COMPACT[f"edges-P{P}-shift{shift}"]
            found |= set(cursors.tolist())
            over = (cursors.reshape(P, NS) > subcap).any(axis=1)
            refused, kept = refused or over.any(), kept or not over.all()
        assert found == set(M.EDGES(M.HAND_SUBCAP)) and refused
        assert kept or P == 1   # (a refused owner next to one that is not)
    assert set(M.WORLDS) == {1, 2, 3, 5, 7, 8}


CAPACITY = M.capacity_cases()


@pytest.mark.parametrize("name", list(CAPACITY))
def test_capacity_model(name):
    P, subcap, cursors, seed, owner, total = CAPACITY[name]
    rt_fp, rt_src = M.routed(P, subcap, seed)
    totals = cursors.reshape(P, NS).sum(axis=1)
    assert cursors.max() <= subcap and totals[owner] == total and all(totals[t] < total for t in range(P) if t != owner)
    for cap, refused in ((total + 1, False), (total, True)):
        fp, src, err, over = M.compact_packed(P, cursors, rt_fp, rt_src, subcap, cap)
        nfp, nsrc, nerr, nover = naive_compact_packed(P, cursors, rt_fp, rt_src, subcap, cap)
        assert fp.tolist() == nfp and src.tolist() == nsrc and err == nerr and over.tolist() == nover
        assert over.tolist() == [refused and t == owner for t in range(P)] and err == (M.DEV_EROUTE if refused else 0)


def test_capacity_cases_cover_first_middle_and_last():
    assert {n.split("-")[1] for n in CAPACITY} == {"first", "middle", "last"}
    for P in (3, 5, 7, 8):
        assert {CAPACITY[f"P{P}-{w}"][4] for w in ("first", "middle", "last")} == {0, P // 2, P - 1}


# --------------------------------------------------------------------------------------------------------------------------- the answers
ANSWERS = M.answer_cases()


@pytest.mark.parametrize("P", M.WORLDS)
def test_answers_model(P):
    for name, (p, off, answers, pend) in ANSWERS.items():
        if p != P:
            continue
        new_src, ends = M.compact_new(P, answers, off, pend)
        nnew, nends = naive_compact_new(P, answers, off, pend)
        assert new_src.tolist() == nnew and ends.tolist() == nends, name
        cnt = M.counts_of(ends)
        if cnt.sum():
            assert M.send_parents(P, new_src, off, cnt, 0x12345).tolist() == naive_send_parents(P, new_src, off, cnt, 0x12345), name


def test_the_answer_cases_are_what_the_issue_lists():
    for P in M.WORLDS:
        mine = {n: c for n, c in ANSWERS.items() if c[0] == P}
        lengths = lambda c: np.diff(c[1][:P + 1].astype(np.int64))   # noqa: E731
        per_owner = lambda c: [c[2][int(c[1][t]):int(c[1][t + 1])] for t in range(P)]   # noqa: E731
        assert not mine[f"P{P}-all-0"][2].any() and mine[f"P{P}-all-1"][2].all()
        for pat, pos in (("first-only", 0), ("last-only", -1)):
            for a in per_owner(mine[f"P{P}-{pat}"]):
                assert a.sum() == 1 and a[pos] == 1
        rnd = mine[f"P{P}-random"][2]
        assert 0.3 < rnd.mean() < 0.7
        assert (mine[f"P{P}-random-bytes"][2] > 1).any()
        if P >= 2:   # an empty range in every place, behind a range that is not empty
            empties = {t for n, c in mine.items() if "-empty-" in n for t in np.flatnonzero(lengths(c) == 0)}
            assert {0, P - 1} <= empties and (P < 3 or P // 2 in empties)
            assert any(lengths(c)[t] == 0 and lengths(c)[t - 1] > 0 and c[2][int(c[1][t]) - 1] for c in mine.values() for t in range(1, P))
        if P >= 3:   # an owner whose every answer is 0 between two that have some
            for quiet in range(1, P - 1):
                a = per_owner(mine[f"P{P}-owner-{quiet}-all-0"])
                assert not a[quiet].any() and len(a[quiet]) and a[quiet - 1].any() and a[quiet + 1].any()
        kept = {int(k) for n, c in mine.items() if "-counts-" in n for k in M.counts_of(M.compact_new(P, c[2], c[1], c[3])[1])}
        assert kept >= set(M.BLOCK_COUNTS)
        ends = {int(o) for c in mine.values() for o in c[1][1:P + 1]}
        assert any(o and o % 64 == 0 for o in ends) and any(o and o % 256 == 0 for o in ends)
        # a 1 right behind an owner boundary and one right in front of it: what an off-by-one there would move
        assert P == 1 or any(c[2][int(c[1][t])] and c[2][int(c[1][t]) - 1] for c in mine.values() for t in range(1, P) if 0 < c[1][t] < len(c[2]))
        for c in mine.values():   # source words: slot and column bits both in use, none of them the pre-fill
            assert (c[3] != M.FILL32).all()
        assert any((c[3] >> 24).max() > 127 and (c[3] & 0xffffff).max() > (1 << 23) for c in mine.values())


# ------------------------------------------------------------------------------------------------------------------ blocks and the arena
@pytest.mark.parametrize("words", [1, 2, 16, 24])
def test_block_layout_model(words):
    rng = np.random.default_rng(words)
    for n in (0, 1, 63, 64, 65, 128, 130):
        states = rng.integers(1, 1 << 63, size=(n, words)).astype(np.uint64)
        buf = M.blocked(states, words)
        assert buf.tolist() == naive_blocked(states, words)
        back, pad = M.unblocked(buf, n, words)
        assert (back == states).all() and not pad.any() and len(pad) == -n % 64
    per_owner = [rng.integers(1, 1 << 63, size=(n, words)).astype(np.uint64) for n in (65, 0, 64, 1)]
    buf = M.send_blocks(per_owner, words)
    assert buf.tolist() == sum((naive_blocked(s, words) for s in per_owner), [])
    for (got, pad), want in zip(M.split_blocks(buf, [65, 0, 64, 1], words), per_owner):
        assert (got == want).all() and not pad.any()


INGEST = M.ingest_cases()


@pytest.mark.parametrize("name", list(INGEST))
def test_ingest_model(name):
    words, n, nxt, cap, seed = INGEST[name]
    arena, parent, recv = M.ingest_input(words, n, nxt, cap, seed)
    assert nxt % 64 and len(np.unique(recv)) == len(recv)
    a2, p2, nxt2, err = M.ingest(words, arena, cap, nxt, recv, n, parent)
    over = nxt + n > cap
    assert (nxt2, err) == ((nxt, M.DEV_EARENA) if over else (nxt + n, 0)) == M.bump(nxt, n, cap)
    for idx in range(len(arena) // words):
        j = idx - nxt
        if 0 <= j < n and idx < cap:
            assert naive_arena_get(a2, words, idx) == [int(recv[(j // 64) * words * 64 + w * 64 + j % 64]) for w in range(words)]
            assert p2[idx] == M.NOT_LOCAL
        else:
            assert naive_arena_get(a2, words, idx) == [M.FILL64] * words and (idx >= cap or p2[idx] == M.FILL32)
    got = M.gather_states(words, a2, nxt, min(n, cap - nxt))
    assert got.tolist() == sum((naive_arena_get(a2, words, nxt + j) for j in range(min(n, cap - nxt))), [])


def test_the_ingest_cases_are_what_the_issue_lists():
    assert {(c[0], c[1]) for c in INGEST.values()} >= {(w, n) for w in (1, 2, 16, 24) for n in (1, 63, 64, 65, 130)}
    words, n, nxt, cap, _ = INGEST["one-past-the-cap"]
    assert nxt + n == cap + 1
    words, n, nxt, cap, _ = INGEST["exact-fit"]
    assert nxt + n == cap


def test_parent_words_model():
    for name, (words, src_rank, nxt, length) in M.parent_cases().items():
        n = len(words)
        assert n <= nxt < length and nxt % 64
        assert (words >> np.uint64(32)).any() and (words & np.uint64(0xffff)).all()
        parent, pslot, prank = np.full(length, M.FILL32, np.uint32), np.full(length, M.FILL16, np.uint16), np.full(length, M.FILL8, np.uint8)
        p2, s2, r2 = M.ingest_parents(words, src_rank, nxt, parent, pslot, prank)
        for i in range(length):
            j = i - (nxt - n)
            if 0 <= j < n:
                assert (int(p2[i]), int(s2[i]), int(r2[i])) == ((int(words[j]) // 65536) % (1 << 32), int(words[j]) % 65536, src_rank)
            else:
                assert (int(p2[i]), int(s2[i]), int(r2[i])) == (M.FILL32, M.FILL16, M.FILL8)
    assert {len(c[0]) for c in M.parent_cases().values()} == {1, 64, 65}


# ------------------------------------------------------------------------------------------------- the cases of the step calls' tests
def test_the_mutants_are_single_edits_of_the_kernels():
    from test_gpu_exchange import MUTANTS
    import testlib
    assert len(MUTANTS) >= 4
    for old, new in MUTANTS.values():
        testlib.mutant_texts(("engine_kernels.h", old, new))   # (asserts it)


@pytest.mark.parametrize("name", list(__import__("shardref").CASES))
def test_the_step_cases_have_what_their_assertions_need(name):
    """tests/test_gpu_shard_steps.py, established on the host: at least two owners receive more than 64 candidates, at least one
    owner's count is no multiple of 64, no two distinct candidate states share a fingerprint.  Candidates per owner (rank r's own are
    probed locally): raft P1 r0 [2590]; raft P3 r1 [275, 199, 317]; raft P8 r0 [128, 100, 152, 170, 76, 140, 91, 48]; raft P8 r7
    [64, 154, 174, 117, 138, 101, 18, 163]; ssi P3 r1 [258, 368, 254]"""
    import shardref as R
    spec, params, P, r, min_frontier = R.CASES[name]
    E, sizes, seen, share = R.host_case(name)
    assert sizes[-1] >= min_frontier > sizes[-2] and len(share) == len(E.frontier) <= 1 << 12   # one chunk
    remote = [n for t, n in enumerate(E.per_owner) if t != r]
    assert P == 1 or sum(n > 64 for n in remote) >= 2
    assert any(n % 64 for n in E.per_owner) and not E.clash
    assert E.local_new and len(E.local_new) < len(E.routed[r])   # some of the rank's own candidates are new, some are not
    # a fingerprint that several (state, slot) pairs generate: what the wavefront's filter may drop before routing
    assert any(n > 1 for t in range(P) if t != r for n in E.routed[t].values()) or P == 1
    expected = {"raft-P1-r0": [2590], "raft-P3-r1": [275, 199, 317], "raft-P8-r0": [128, 100, 152, 170, 76, 140, 91, 48],
                "raft-P8-r7": [64, 154, 174, 117, 138, 101, 18, 163], "ssi-P3-r1": [258, 368, 254]}
    assert E.per_owner == expected[name]


def test_the_step_cases_are_the_ranks_the_issue_names():
    import shardref as R
    assert {(c[0], c[2], c[3]) for c in R.CASES.values()} == {("raft", 1, 0), ("raft", 3, 1), ("raft", 8, 0), ("raft", 8, 7), ("ssi", 3, 1)}
