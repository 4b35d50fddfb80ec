"""The exchange kernels of the sharded engine (engine_kernels.h, "sharded step kernels") against tests/xchgmodel.py, on arrays that no
search produced, launched through tests/xchgshim.py with the engine's grids.  Every comparison is exact and covers the whole output
buffer: what the kernel must not write holds its pre-fill, and the guard zones around every written buffer are intact.
tests/test_exchange_reference.py checks the model and that these cases hold the edges they are meant to hold.  At the end: four edits of
engine_kernels.h, each caught by a test here that the product passes."""
import functools

import numpy as np
import pytest

import xchgmodel as M
import xchgshim as X
from testlib import build_mutants, mutant_tree, survives

pytestmark = pytest.mark.gpu

COMPACT, CAPACITY, ANSWERS, INGEST = M.compact_cases(), M.capacity_cases(), M.answer_cases(), M.ingest_cases()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert not len(bad), f"{what}: {len(bad)} differ, the first at {bad[0]}: {got[bad[0]]:#x}, expected {want[bad[0]]:#x}"


# ------------------------------------------------------------------------------------------------------------------------ the compaction
def check_exact(name, L=None):
    P, subcap, cursors, seed = COMPACT[name]
    rt_fp, rt_src = M.routed(P, subcap, seed)
    fp, src, intact = X.compact_buckets(P, cursors, rt_fp, rt_src, subcap, L=L)
    wfp, wsrc, _ = M.compact_exact(P, cursors, rt_fp, rt_src, subcap)
    same(fp, wfp, f"{name}: send_fp")
    same(src, wsrc, f"{name}: pend_src")
    assert intact, name


def check_packed(P, subcap, cursors, seed, cap, name, L=None):
    rt_fp, rt_src = M.routed(P, subcap, seed)
    fp, src, err, intact = X.compact_packed(P, cursors, rt_fp, rt_src, subcap, cap, L=L)
    wfp, wsrc, werr, over = M.compact_packed(P, cursors, rt_fp, rt_src, subcap, cap)
    same(fp.reshape(P, cap)[:, 0], wfp.reshape(P, cap)[:, 0], f"{name}: the count words")
    same(fp, wfp, f"{name}: send_fp")
    same(src, wsrc, f"{name}: pend_src")
    assert err == werr, name
    assert intact, name
    return over


@pytest.mark.parametrize("name", list(COMPACT))
def test_compact_buckets(name):
    check_exact(name)


@pytest.mark.parametrize("name", list(COMPACT))
def test_compact_packed(name):
    P, subcap, cursors, seed = COMPACT[name]
    over = check_packed(P, subcap, cursors, seed, M.packed_cap(P, cursors, subcap), name)
    assert over.any() == bool((cursors > subcap).any())


def check_capacity(name, L=None):
    P, subcap, cursors, seed, owner, total = CAPACITY[name]
    over = check_packed(P, subcap, cursors, seed, total + 1, f"{name}: cap = total + 1", L=L)
    assert not over.any()
    over = check_packed(P, subcap, cursors, seed, total, f"{name}: cap = total", L=L)
    assert over.tolist() == [t == owner for t in range(P)]


@pytest.mark.parametrize("name", list(CAPACITY))
def test_packed_capacity(name):
    check_capacity(name)


# --------------------------------------------------------------------------------------------------------------------------- the answers
def check_answers(P, L=None):
    for name, (p, off, answers, pend) in ANSWERS.items():
        if p != P:
            continue
        new_src, ends, intact = X.compact_new(P, answers, off, pend, L=L)
        wnew, wends = M.compact_new(P, answers, off, pend)
        same(ends, wends, f"{name}: ends")
        same(new_src, wnew, f"{name}: new_src")
        assert intact, name
        cnt = M.counts_of(wends)
        if cnt.sum():   # the moved states' parents, from the list as it should be (its pre-fill where nothing belongs: never to be read)
            for chunk_base in (0, 0x12340, (1 << 32) - (1 << 24) - 64):
                words, intact = X.send_parents(P, wnew, off, cnt, chunk_base, L=L)
                same(words[:cnt.sum()], M.send_parents(P, wnew, off, cnt, chunk_base), f"{name}: send_parents")
                assert (words[cnt.sum():] == M.FILL64).all() and intact, name


@pytest.mark.parametrize("P", M.WORLDS)
def test_compact_new_and_send_parents(P):
    check_answers(P)


# ------------------------------------------------------------------------------------------------------------------ blocks and the arena
def check_ingest(name, L=None):
    words, n, nxt, cap, seed = INGEST[name]
    arena, parent, recv = M.ingest_input(words, n, nxt, cap, seed)
    warena, wparent, wnext, werr = M.ingest(words, arena, cap, nxt, recv, n, parent)
    got_next, err, intact = X.ingest(words, arena, cap, nxt, recv, n, parent, L=L)
    assert (got_next, err) == (wnext, werr), name
    same(arena, warena, f"{name}: the arena")
    same(parent, wparent, f"{name}: the parent column")
    assert intact, name
    return arena


@pytest.mark.parametrize("name", list(INGEST))
def test_ingest(name):
    words, n, nxt, cap, seed = INGEST[name]
    arena = check_ingest(name)
    if nxt + n > cap:   # refused: arena_next stays, and nothing at or beyond the cap was written
        rows = arena.reshape(-1, words, 64).transpose(0, 2, 1).reshape(-1, words)
        assert (rows[cap:] == M.FILL64).all()
    # ... and read back by the gather kernel, from a start that is no block's
    count = min(n, cap - nxt)
    out, intact = X.gather_states(words, arena, nxt, count)
    same(out, M.gather_states(words, arena, nxt, count), f"{name}: gather_states")
    assert intact
    out, intact = X.gather_states(words, arena, 0, len(arena) // words)
    same(out, M.gather_states(words, arena, 0, len(arena) // words), f"{name}: gather_states, all")
    assert intact


def check_parents(L=None):
    for name, (words, src_rank, nxt, length) in M.parent_cases().items():
        parent, pslot, prank = np.full(length, M.FILL32, np.uint32), np.full(length, M.FILL16, np.uint16), np.full(length, M.FILL8, np.uint8)
        wparent, wpslot, wprank = M.ingest_parents(words, src_rank, nxt, parent, pslot, prank)
        assert X.ingest_parents(words, src_rank, nxt, parent, pslot, prank, L=L), name
        same(parent, wparent, f"{name}: parent")
        same(pslot, wpslot, f"{name}: pslot")
        same(prank, wprank, f"{name}: prank")


def test_ingest_parents():
    check_parents()


@pytest.mark.parametrize("on_device", [False, True])
def test_bump_arena_next(on_device):
    for nxt, n, cap in ((37, 65, 200), (37, 65, 102), (37, 65, 101), (0, 0, 1), (100, 1, 100), (5, (1 << 32) - 1, 1 << 33)):
        assert X.bump_arena_next(nxt, n, on_device, cap) == M.bump(nxt, n, cap), (nxt, n, cap)


# ---------------------------------------------------------------------------------------------------------------- mutants of the device code
# Four edits of engine_kernels.h.  Each changes a compared value or a position by one inside a buffer that the shim allocates with 64
# elements of slack on either side, never an arena column, a source word, a loop bound or a grid:
#   * owner_of_index keeps a range's successor's first position: that candidate's source lands behind the wrong owner's kept sources
#     (a position <= its own, so inside new_src);
#   * a packed bucket of exactly `cap` candidates is accepted: its last candidate lands on the next owner's count word (the last
#     owner's: on the first word of the guard zone);
#   * a range's end is read one position late: an end is one too large where the next range starts with a 1 (the last range reads the
#     guard zone of the scan, an input), and the sources of the owners behind it land one position early (owner 1's at worst at off - 1,
#     in the guard zone in front when off is 0);
#   * the parent index is shifted by 15: a value.
MUTANTS = {
    "owner-boundary": ("i >= o.off[t + 1]", "i > o.off[t + 1]"),
    "packed-cap": ("over |= total + 1 > cap", "over |= total > cap"),
    "range-end": ("offs.off[t + 1] ? incl[offs.off[t + 1] - 1] : 0", "offs.off[t + 1] ? incl[offs.off[t + 1]] : 0"),
    "parent-shift": ("recv_parents[j] >> 16", "recv_parents[j] >> 15"),
}


@functools.lru_cache(maxsize=None)
def mutant_libraries():
    top = X.SHIM_DIR / "_build" / "mutants"   # (kept between runs: an unchanged mutant stays fresh)
    return build_mutants(MUTANTS, lambda name: X.build(csrc=mutant_tree(top, name, ("engine_kernels.h", *MUTANTS[name])), out=top / name))


@pytest.fixture(scope="module")
def mutants():
    return {name: X.load(so) for name, so in mutant_libraries().items()}


def test_a_moved_owner_boundary_is_caught(mutants):
    assert not survives(lambda: check_answers(3, L=mutants["owner-boundary"]))
    check_answers(3)


def test_a_full_packed_bucket_is_caught(mutants):
    for name in ("P3-first", "P3-middle", "P3-last"):
        assert not survives(lambda: check_capacity(name, L=mutants["packed-cap"])), name
        check_capacity(name)


def test_a_late_range_end_is_caught(mutants):
    assert not survives(lambda: check_answers(5, L=mutants["range-end"]))
    check_answers(5)


def test_another_parent_shift_is_caught(mutants):
    assert not survives(lambda: check_parents(L=mutants["parent-shift"]))
    check_parents()
