"""The one validation of a liveness query (tla_rust_amd/csrc/live_query.h: live_query_error) and its normalisation, on the host: the
header is built with g++ into tests/_queryshim and driven with a table of queries — a good one of each of the six kinds the C ABI has,
then every refusal, one defect per row, with the words the engine, the graph passes and the test drivers all report it in.

The shapes: 3 process instances; a table of 4 units and 3 conjuncts; 2 predicates."""
import ctypes as C

import pytest

import helpers
import testlib

SHIM_DIR = helpers.ROOT / "tests" / "_queryshim"
CSRC = helpers.ROOT / "tla_rust_amd" / "csrc"
LEADS_TO, INF_OFTEN, EVENTUALLY, STABLE = range(4)
NPRED = 2
ALL = 0b111


class FairUnits(C.Structure):
    """mc_fair_units"""
    _fields_ = [("nunits", C.c_int32), ("nconj", C.c_int32), ("of_unit", C.c_uint64 * 128), ("weak_mask", C.c_uint64), ("strong_mask", C.c_uint64)]


def build():
    return testlib.build_library(SHIM_DIR / "_build" / "libqueryshim.so", testlib.host_argv("-O1", "-I", CSRC, SHIM_DIR / "queryshim.cpp"),
                                 [SHIM_DIR / "queryshim.cpp"] + testlib.product_deps(CSRC))


@pytest.fixture(scope="module")
def shim():
    L = C.CDLL(str(build()))
    L.queryshim_check.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(FairUnits), C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t,
                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


def table(nunits=4, nconj=3, of_unit=(0b001, 0b010, 0b101, 0b000), weak=0b011, strong=0b100):
    """units 0 and 1 in one weak conjunct each, unit 2 in the first and in a strong one of its own, unit 3 in none"""
    fu = FairUnits()
    fu.nunits, fu.nconj, fu.weak_mask, fu.strong_mask = nunits, nconj, weak, strong
    for u, m in enumerate(of_unit):
        fu.of_unit[u] = m
    return fu


def ask(L, refine=False, weak=0b011, strong=0, fu=None, kind=-1, p=-1, q=-1, npred=NPRED, all_mask=ALL):
    """(the refusal or None, the normalised p, the normalised q)"""
    msg = C.create_string_buffer(512)
    po, qo = C.c_int(99), C.c_int(99)
    refused = L.queryshim_check(int(refine), all_mask, weak, strong, None if fu is None else C.byref(fu), kind, p, q, npred, msg, len(msg), C.byref(po), C.byref(qo))
    text = msg.value.decode()
    assert bool(refused) == bool(text)
    return (text or None), po.value, qo.value


# what each of the six C entries asks, well formed
GOOD = {
    "liveness": dict(),
    "liveness_check": dict(kind=LEADS_TO, p=0, q=1),
    "liveness_strong": dict(refine=True, weak=0b001, strong=0b110),
    "liveness_check_strong": dict(refine=True, weak=0b001, strong=0b110, kind=STABLE, p=1),
    "liveness_units": dict(fu=table()),
    "liveness_check_units": dict(fu=table(), kind=INF_OFTEN, q=0),
}
NO_PRED = "a predicate index the program does not have (it has %d predicates)"
# one defect each: (the query, the refusal word for word)
BAD = {
    "a weak mask with an instance beyond `all`": (dict(weak=0b1011), "the fairness mask names a process instance the program does not have"),
    "a strong mask with an instance beyond `all`": (dict(refine=True, weak=0b001, strong=0b1010), "a fairness mask names a process instance the program does not have"),
    "overlapping process masks": (dict(refine=True, weak=0b011, strong=0b010), "the weak and the strong mask overlap (a strongly fair process is weakly fair already)"),
    "overlapping conjunct masks": (dict(fu=table(weak=0b111)), "the weak and the strong mask overlap (a conjunct is WF or SF)"),
    "nunits = 128": (dict(fu=table(nunits=128)), "128 units (at most 127)"),
    "nconj = 65": (dict(fu=table(nconj=65)), "65 conjuncts (at most 64)"),
    "a mask bit at nconj": (dict(fu=table(weak=0b1011)), "a fairness mask names a conjunct beyond nconj"),
    "of_unit[0] with a bit at nconj": (dict(fu=table(of_unit=(0b1001, 0b010, 0b101, 0))), "of_unit[0] names a conjunct beyond nconj"),
    "of_unit[nunits] non-zero": (dict(fu=table(of_unit=(0b001, 0b010, 0b101, 0, 0b001))), "of_unit[4] names conjuncts for a unit beyond nunits"),
    "kind 4": (dict(kind=4, p=0, q=1), "unknown kind 4"),
    "kind -2": (dict(kind=-2, p=0, q=1), "unknown kind -2"),
    "p = -1 where P ~> Q needs it": (dict(kind=LEADS_TO, p=-1, q=1), NO_PRED % NPRED),
    "q = npred where []<>Q needs it": (dict(kind=INF_OFTEN, q=NPRED), NO_PRED % NPRED),
    "npred = 33": (dict(kind=LEADS_TO, p=0, q=1, npred=33), NO_PRED % 33),
}
# the index a kind does not read is neither checked nor kept: (the query, the normalised (p, q))
UNREAD = {
    "[]<>Q ignores p": (dict(kind=INF_OFTEN, p=7, q=0), (-1, 0)),
    "<>Q ignores p": (dict(kind=EVENTUALLY, p=7, q=1), (-1, 1)),
    "<>[]P ignores q": (dict(kind=STABLE, p=0, q=7), (0, -1)),
}


@pytest.mark.parametrize("name", GOOD)
def test_a_good_query_of_every_kind_is_accepted(shim, name):
    why, p, q = ask(shim, **GOOD[name])
    assert why is None, (name, why)
    want = GOOD[name]
    assert (p, q) == (want.get("p", -1), want.get("q", -1))   # (what the kind reads is kept; Termination reads neither)


@pytest.mark.parametrize("name", BAD)
def test_every_defect_is_refused_in_the_engines_words(shim, name):
    query, words = BAD[name]
    why, _, _ = ask(shim, **query)
    assert why == words, (name, why)


@pytest.mark.parametrize("name", UNREAD)
def test_an_index_the_kind_does_not_read_is_ignored_and_becomes_minus_one(shim, name):
    query, want = UNREAD[name]
    for entry in (dict(), dict(refine=True, weak=0b001, strong=0b110), dict(fu=table())):
        why, p, q = ask(shim, **dict(entry, **query))
        assert why is None and (p, q) == want, (name, entry, why, p, q)


def test_the_table_decides_the_conjuncts_not_the_callers_all(shim):
    """a query by units is judged against nconj: a mask bit below nconj is good whatever `all` the caller passed"""
    assert ask(shim, fu=table(), all_mask=0)[0] is None
    assert ask(shim, fu=table(nconj=64, weak=1 << 63 | 0b011))[0] is None   # (64 conjuncts: every bit is one)
