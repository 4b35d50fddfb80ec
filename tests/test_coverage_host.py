"""What -coverage counts, on the host (tla_rust_amd/csrc/coverage.h through tests/_covshim, no GPU), against the ORACLE'S STATE GRAPH:
the per-(state, slot) classification and the action mapping the device kernels run (engine_coverage.h) are run here over every state
of the graph, and the per-action sums must be the oracle's edge counts per action NAME (oracle/bfs.c's edge dump: one line per
successor the search generates, labelled with the action that generated it).  The states searched are the oracle's dump, text by text.

Mutants of the headers (test_mutants_are_killed builds each and asserts that `suite` fails) and what kills each:
  selfloop-dropped      a self loop does not count                      raft: Restart / DuplicateMessage ... are short
  out-of-model-dropped  an out-of-model successor does not count        raft (its CONSTRAINT bounds the model)
  flagged-dropped       a failed Assert does not count                  the README's pcal_intro: C is short
  ids-swapped           atomic_add's Increment and Check swap ids       atomic_add: Increment 1, Check 12
  vote-is-increase      Voting's VoteFor slots counted as IncreaseMaxBal   Voting
"""
from pathlib import Path

import pytest

import covshim
import helpers
import testlib

ROOT = helpers.ROOT
RAFT = [2, 2, 2, 9, 1, 1]
MODELS = [
    ("atomic_add", [3], [3], True),
    ("pcal_intro", [0, 1, 20, 2], [0, 1, 20, 2], True),
    ("pcal_intro", [1, 1, 20, 2], [1, 1, 20, 2], True),          # MoneyInvariant fails
    ("pcal_intro", [1, 0, 20, 2], [1, 0, 20, 2], True),          # the README's Assert fails: flagged successors
    ("raft", RAFT, helpers.raft_oracle_params(RAFT), True),      # 2 servers: self loops, out-of-model successors
    ("ssi", [2, 2, 127, 0], [2, 2, 127, 0], True),               # 2 x 2, no SYMMETRY
    ("paxos", [1, 3, 2, 2, 1, 0, 1], [1, 3, 2, 2, 1, 0, 1], False),  # Voting
]
IDS = [f"{s}{p}" for s, p, _, _ in MODELS]


def check_model(tmp, spec, params, oparams, deadlock, L=None):
    g = covshim.OracleGraph(spec, oparams, tmp, check_deadlock=deadlock)
    r = covshim.search(spec, params, dump=tmp / "host_states.txt", L=L)
    want = g.generated()
    print(spec, params, "generated", r["generated"], "oracle", dict(want))
    assert set(want) <= set(r["generated"]), (set(want) - set(r["generated"]), "an action name the oracle has and the model's list has not")
    for name, n in r["generated"].items():
        assert n == want[name], f"{spec}{params}: generated[{name}] = {n}, the oracle's graph has {want[name]} such edges"
    assert sum(r["generated"].values()) == g.counters["generated"] == len(g.edges)
    # every state of the oracle's dump was searched, and nothing else
    assert helpers.read_dump(tmp / "host_states.txt") == helpers.read_dump(tmp / "cov_states.txt")
    lower, upper, stored = g.distinct_bounds()
    assert r["states"] == stored == g.counters["distinct"] == sum(r["distinct"].values())
    for name, n in r["distinct"].items():
        assert lower[name] <= n <= upper[name], (name, lower[name], n, upper[name])
        assert n == 0 or r["generated"][name] > 0


@pytest.mark.parametrize("spec,params,oparams,deadlock", MODELS, ids=IDS)
def test_host_counts_are_the_edge_counts_of_the_oracles_graph(tmp_path, spec, params, oparams, deadlock):
    check_model(tmp_path, spec, params, oparams, deadlock)


def test_zero_rows_are_listed(tmp_path):
    """pcal_intro variant 0 has no labels A and B: their rows are there, 0 : 0 (the vacuous-action signal)"""
    r = covshim.search("pcal_intro", [0, 1, 20, 2])
    assert list(r["generated"]) == ["Init", "Transfer", "A", "B", "C", "Terminating"]
    assert r["generated"]["A"] == r["generated"]["B"] == 0 and r["distinct"]["A"] == r["distinct"]["B"] == 0
    assert list(covshim.search("paxos", [1, 3, 2, 2, 1, 0, 1])["generated"]) == ["Init", "IncreaseMaxBal", "VoteFor"]


def test_compiled_program_rows_are_the_labels(tmp_path):
    """a compiled PlusCal program: one row per label, none for "Done", one for the terminating disjunct; the dead label is 0 : 0"""
    text = (ROOT / "specs" / "pluscal" / "dead_label.tla").read_text()
    host = helpers.ShimProgram(text, invariants=["Bounded", "OneAtATime"])
    try:
        r = covshim.search("pcal", host.params)
    finally:
        host.close()
    assert list(r["generated"]) == ["Init", "Enter", "Work", "Check", "Panic", "Leave", "Terminating"]
    assert r["generated"]["Panic"] == 0 and r["distinct"]["Panic"] == 0
    assert all(n > 0 for name, n in r["generated"].items() if name != "Panic")
    assert sum(r["distinct"].values()) == r["states"]


# ------------------------------------------------------------------------------------------------ mutants
# name: (header, its text, the replacement, the model of MODELS that must fail, what the failure must say)
MUTANTS = {
    "selfloop-dropped": ("coverage.h", "return (st & ST_ENABLED) != 0;", "return (st & ST_ENABLED) != 0 && !(st & ST_SELFLOOP);", 4, "generated["),
    "out-of-model-dropped": ("coverage.h", "return (st & ST_ENABLED) != 0;", "return (st & ST_ENABLED) != 0 && !(st & ST_OUT_OF_MODEL);", 4, "generated["),
    "flagged-dropped": ("coverage.h", "return (st & ST_ENABLED) != 0;", "return (st & ST_ENABLED) != 0 && !(st & (ST_ASSERT | ST_SPECERR));", 3, "generated[C]"),
    "ids-swapped": ("spec_pluscal.h", "return slot == 0 ? 1 : slot <= p.n ? 0 : 2;", "return slot == 0 ? 0 : slot <= p.n ? 1 : 2;", 0, "generated[Increment] = 1,"),
    "vote-is-increase": ("spec_paxos.h", "if (p.kind == 1) return slot < p.na * p.nb ? 0 : 1;", "if (p.kind == 1) return 0;", 6, "generated[IncreaseMaxBal]"),
}


def test_mutants_are_killed(tmp_path):
    helpers.build_shim()

    def build(name):
        return covshim.build_covshim(csrc=testlib.mutant_tree(tmp_path, name, MUTANTS[name][:3]), out=tmp_path / name / "_build")
    for name, so in testlib.build_mutants(MUTANTS, build).items():
        _, _, _, model, says = MUTANTS[name]
        d = tmp_path / name / "run"
        d.mkdir()
        with pytest.raises(AssertionError) as e:
            check_model(d, *MODELS[model], L=covshim.load(so))
            pytest.fail(f"mutant {name} survives", pytrace=False)
        assert says in str(e.value), (name, str(e.value)[:300])
    # ... and the product's own library passes where they fail
    for model in sorted({m[3] for m in MUTANTS.values()}):
        d = tmp_path / f"product{model}"
        d.mkdir()
        check_model(d, *MODELS[model])
