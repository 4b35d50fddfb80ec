"""Simulation mode's walk on the host (tla_rust_amd/csrc/sim_walk.h through tests/_simshim, no GPU): every state a walk reaches is a
state the BFS stores, at a BFS level no deeper than its place in the walk; the walks cover a small model; they find the README model's
assertion failure along a behaviour of the model.

These are checks of the state SET.  That consecutive states are transitions of the oracle's graph, that a walk ends for the reason the
graph gives, its counters and the uniformity of its choices are tests/test_simulate_graph.py's (reference: tests/simgraph.py)."""
import pytest

import helpers
import simwalk

MODELS = [
    ("atomic_add", [3], [3]),
    ("atomic_add", [4], [4]),
    ("pcal_intro", [0, 1, 20, 2], [0, 1, 20, 2]),
    ("pcal_intro", [1, 1, 20, 2], [1, 1, 20, 2]),
    ("raft", [2, 2, 2, 9, 1, 1], helpers.raft_oracle_params([2, 2, 2, 9, 1, 1])),
    ("ssi", [2, 2, 127, 0], [2, 2, 127, 0]),
    ("paxos", [1, 3, 2, 2, 1, 0, 1], [1, 3, 2, 2, 1, 0, 1]),   # Voting over MCBallot = 0..1 (deadlocks; no SYMMETRY: the oracle prints other orbit representatives)
]


@pytest.mark.parametrize("spec,params,oparams", MODELS, ids=[f"{s}{p}" for s, p, _ in MODELS])
@pytest.mark.parametrize("deadlock", [True, False])
def test_walk_states_are_bfs_states(tmp_path, spec, params, oparams, deadlock):
    levels = simwalk.oracle_levels(spec, oparams, tmp_path / "oracle.txt", check_deadlock=deadlock)
    r = simwalk.walks(spec, params, seed=12345, n=3000, depth=60, deadlock=deadlock, dump=str(tmp_path / "walks.txt"))
    states = simwalk.walk_dump(tmp_path / "walks.txt")
    assert len(states) == r["steps"] > 3000
    bad = [(t, s) for t, s in states if s not in levels or levels[s] > t]
    assert not bad, bad[:3]
    assert r["walks_done"] == 3000 and all(w["end"] in simwalk.END for w in r["walks"])
    assert all(len(w["slots"]) == w["len"] - 1 for w in r["walks"])
    assert r["generated"] >= r["steps"]
    if r["viol"] is not None:   # the run's violation is in the lowest-indexed walk that ended on one
        first = min(k for k, w in enumerate(r["walks"]) if w["end"] == 2)
        assert simwalk.key_walk(r["viol"]) == first


def test_walks_cover_atomic_add(tmp_path):
    """atomic_add with N = 3: 17 reachable states; a thousand seeded walks meet all of them"""
    levels = simwalk.oracle_levels("atomic_add", [3], tmp_path / "oracle.txt")
    simwalk.walks("atomic_add", [3], seed=7, n=1000, depth=100, dump=str(tmp_path / "walks.txt"))
    seen = {s for _, s in simwalk.walk_dump(tmp_path / "walks.txt")}
    assert seen == set(levels)


def test_walks_are_a_function_of_seed_and_index():
    a = simwalk.walks("raft", [2, 2, 2, 9, 1, 1], seed=99, n=50, depth=40)
    b = simwalk.walks("raft", [2, 2, 2, 9, 1, 1], seed=99, n=20, depth=40, first=30)
    assert a["walks"][30:] == b["walks"]
    c = simwalk.walks("raft", [2, 2, 2, 9, 1, 1], seed=100, n=50, depth=40)
    assert a["walks"] != c["walks"]


def test_readme_pcal_intro_violation_is_a_behaviour(tmp_path):
    """The README's pcal_intro (labels A: / B:) fails its assertion; the walk that finds it is a path of the state graph"""
    params = [1, 0, 20, 2]   # specs/readme_variant/pcal_intro.cfg checks no invariant
    levels = simwalk.oracle_levels("pcal_intro", params, tmp_path / "oracle.txt")
    o = helpers.oracle_run("pcal_intro", params)
    assert o["verdict"] == "assert"
    r = simwalk.walks("pcal_intro", params, seed=1, n=2000, depth=100)
    assert r["viol"] is not None and simwalk.key_kind(r["viol"]) == 2   # Assert
    w = simwalk.key_walk(r["viol"])
    assert r["walks"][w]["end"] == 2 and all(x["end"] != 2 for x in r["walks"][:w])
    one = simwalk.walks("pcal_intro", params, seed=1, n=1, depth=100, first=w, rows_walk=w)
    n = one["walks"][0]["len"]
    texts = [simwalk.fmt("pcal_intro", params, row).replace("\n", " ") for row in one["rows"][:n]]
    # every state is reachable no deeper than its position; consecutive states are one step of the spec apart (BFS level grows by
    # at most one along the walk, and the successor of state k by slot k is state k + 1: the shim's apply is what the kernel runs)
    assert all(t in levels and levels[t] <= k + 1 for k, t in enumerate(texts))
    assert all(levels[texts[k + 1]] <= levels[texts[k]] + 1 for k in range(n - 1))
    # the state the assertion fails in: alice's account is negative, and the failing process is at label C
    assert "alice_account = -" in texts[-1]
    failing = simwalk.key_slot(r["viol"])
    assert texts[-1].split("pc = <<")[1].split(">>")[0].split(", ")[failing] == '"C"'
