"""Simulation mode on the GPU against the oracle's state graph (tests/simgraph.py), at the shapes tests/test_gpu_simulate.py leaves out:
few walks and partial wavefronts, depths around one launch's 16 events, walks of the second round (index >= 2^18), and the device's
own counterexample rows as paths of the graph.  Device walks are first compared slot by slot with the host's (same_as_host); the host's
rows of those walks then go through the graph reference, so a mistake shared by host and device (one sim_walk.h) is seen too."""
import pytest

import helpers
import simgraph
from test_gpu_simulate import CAS, ROOT, SMALL, amd, compiled, same_as_host  # noqa: F401
from test_simulate_graph import RAFT, check, graph, raft_slice

pytestmark = pytest.mark.gpu
ROUND = 1 << 18
KIND = {"invariant": simgraph.VK_INVARIANT, "assert": simgraph.VK_ASSERT, "deadlock": simgraph.VK_DEADLOCK, "spec-error": simgraph.VK_SPECERR}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_few_walks_and_partial_wavefronts(amd, tmp_path, n):
    same_as_host(amd, "raft", RAFT, RAFT, seed=31, n=n, depth=40)
    check(tmp_path, graph("raft", tuple(helpers.raft_oracle_params(RAFT))), "raft", RAFT, 31, n, 40, True)


@pytest.mark.parametrize("depth", [1, 2, 15, 16, 17, 31, 32, 33])
def test_depths_around_a_launch(amd, tmp_path, depth):
    """one launch advances a walk by 16 events: the first builds state 1, the last of a walk notices its end"""
    for spec, params in (("raft", RAFT), ("pcal_intro", [0, 1, 20, 2])):
        same_as_host(amd, spec, params, params, seed=32, n=300, depth=depth)
        oparams = helpers.raft_oracle_params(params) if spec == "raft" else params
        check(tmp_path, graph(spec, tuple(oparams)), spec, params, 32, 300, depth, True)


def test_walks_of_the_second_round(amd, tmp_path):
    """2^18 + 65 walks, all recorded: the second round (w0 = 2^18, one full and one partial wavefront) slot by slot, and the counters
    of a two-round run"""
    n = ROUND + 65
    r = same_as_host(amd, "atomic_add", [3], [3], seed=33, n=n, depth=8)
    assert r.walks == n
    g = graph("atomic_add", (3,))
    ends, run, _ = check(tmp_path, g, "atomic_add", [3], 33, 65 + 64, 8, True, first=ROUND - 64)
    assert sum(ends.values()) == 129


VIOLATING = [
    ("pcal_intro", [1, 0, 20, 2], "assert", True, 100000, 100),
    ("pcal_intro", [1, 1, 20, 2], "invariant", True, 100000, 100),
    ("paxos", [0, 3, 2, 2, 15, 0, 3], "invariant", False, 100000, 100),
    ("paxos", [1, 3, 2, 2, 1, 0, 1], "deadlock", True, 2000, 100),
]


@pytest.mark.parametrize("spec,params,verdict,deadlock,num,depth", VIOLATING, ids=[f"{v[0]}{v[1]}" for v in VIOLATING])
def test_device_counterexamples_are_paths_of_the_graph(amd, tmp_path, spec, params, verdict, deadlock, num, depth):
    """32 seeds: the device's own rows (mc_engine_trace, mc_state_format) are a path of the oracle's graph that ends in the violation
    the verdict names and meets none before; for every seed, no host walk of a lower index (the 20 000 below it at most, as
    check_violation caps its scan) is a violating walk according to the graph reference"""
    g, inv_on = graph(spec, tuple(params)), simgraph.INV_ON[spec]
    eng = amd.Engine(spec, params, deadlock=deadlock, **SMALL)
    try:
        for seed in range(32):
            r = eng.simulate(num, depth, seed)
            assert r.verdict == verdict, (seed, dict(r))
            texts = [t.replace("\n", " ") for _, t in eng.trace()]
            assert len(texts) == r.trace_len
            succ = None
            if verdict == "invariant" and inv_on == "successor" and len(texts) > 1:
                texts, succ = texts[:-1], texts[-1]
            slot = simgraph.SLOT_NONE if verdict == "deadlock" else simgraph.SLOT_PARENT if verdict == "invariant" and succ is None else 0
            simgraph.check_walk(g, texts, simgraph.END_VIOLATION, depth, deadlock, inv_on,
                                viol=(KIND[verdict], r.violated_invariant if verdict == "invariant" else 0, slot), viol_succ=succ)
            below = min(r.violating_walk, 20000)
            if below:
                ends, _, _ = check(tmp_path, g, spec, params, seed, below, depth, deadlock, first=r.violating_walk - below)
                assert ends[simgraph.END_VIOLATION] == 0
    finally:
        eng.close()


def test_interpreter_and_generated_code_walk_the_evaluators_graph(amd, tmp_path):
    import sys
    sys.path.insert(0, str(ROOT / "oracle"))
    from tla_eval import Checker
    invs, consts = ["NeverTooMany", "SeenIsOld"], {"Workers": 2, "N": 2}
    prog, host = compiled(amd, CAS, ROOT / "specs" / "pluscal" / "cas_counter.cfg", invs, consts)
    try:
        g = simgraph.from_checker(Checker(host.translated(), constants=consts), invariants=invs)
        for jit in (False, True):
            same_as_host(amd, "pcal", prog.params, host.params, seed=6, n=400, depth=33, jit=jit)
        ends, _, _ = check(tmp_path, g, "pcal", host.params, 6, 400, 33, True)
        assert ends[simgraph.END_STUTTER] > 0
    finally:
        prog.close()
        host.close()


def test_a_million_raft_walks_total_what_the_graph_gives(amd):
    """2^20 walks (four rounds) of the two-server raft model: the device's generated / steps / walks / max_depth equal the sums the graph
    reference computes over the host's rows of the same walks, every one of which it judges.  The host part runs in eight fresh
    processes that do not touch the GPU (a slice of 2^16 walks takes one core 4 - 8 s, most of it in Python)."""
    import multiprocessing
    n, depth, seed, piece = 1 << 20, 20, 34, 1 << 16
    eng = amd.Engine("raft", RAFT, **SMALL)
    r = eng.simulate(n, depth, seed)
    eng.close()
    with multiprocessing.get_context("spawn").Pool(8) as pool:
        parts = pool.map(raft_slice, [(seed, first, piece, depth) for first in range(0, n, piece)])
    want = (sum(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts), max(p[3] for p in parts))
    assert (r.verdict, r.generated, r.steps, r.walks, r.max_depth) == ("ok",) + want
