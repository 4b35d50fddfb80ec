"""The engine's own probers — the by-family kernel (raft), the by-pairs kernel with its blind first compare-and-swap and its pipelined copy of
the placement rule (the SI models), the slot-by-slot kernel (atomic_add, pcal_intro) — at seen-set loads that no other test reaches: a
dense table that fits the graph exactly (load >= 0.99: every bucket full in the end, chains that wrap), a dense table at load 0.9, and
the 4-slot form at load 0.8, which the engine only chooses by itself below a third.  Through the C ABI against the oracle's counts, level
by level; chunk_states is small, so a level is many launches into the same table.  Every load is computed from the oracle's count and
asserted.  tests/test_gpu_seenset.py drives seen_insert_t, k_probe, k_insert and seen_find directly."""
import json
import os
import subprocess
import sys

import pytest

import helpers

pytestmark = pytest.mark.gpu
MC_ETABLEFULL = -4
CHUNK = 1 << 10
KEYS = ("distinct", "generated", "depth", "verdict", "levels")

# (spec, engine params): complete graphs of at most 16 384 states — at most 2048 buckets of 8, so a probe visits every bucket
EXACT = {
    "raft": ("raft", [2, 2, 2, 9, 1, 1]),           # 13 634 states, the by-family kernel
    "ssi": ("ssi", [2, 2, 127, 0, 0, 3]),           # 7 419 orbits, the by-pairs kernel
    "ssi_tiny": ("ssi", [2, 1, 127, 0]),            # 569 states: 72 buckets
    "atomic_add": ("atomic_add", [13]),             # 8 193 states, the slot-by-slot kernel
    "pcal_intro": ("pcal_intro", [0, 1, 7, 3]),     # 11 973 states, the same
}
# 30 000 - 300 000 states, complete
LARGER = {
    "raft": ("raft", [2, 3, 2, 9, 1, 1]),           # 88 490 states
    "ssi": ("ssi", [3, 1, 127, 0]),                 # 90 430 states
    "atomic_add": ("atomic_add", [16]),             # 65 537 states
}


@pytest.fixture(scope="module")
def amd():
    import tla_rust_amd
    assert tla_rust_amd.device_count() >= 1, "no HIP device visible"
    return tla_rust_amd


_oracle = {}


def oracle_of(case):
    """the oracle's counts of a case, computed once"""
    spec, params = case
    k = (spec, tuple(params))
    if k not in _oracle:
        helpers.build_oracle()
        _oracle[k] = helpers.oracle_run(spec, helpers.raft_oracle_params(params) if spec == "raft" else params)
        assert _oracle[k]["verdict"] == "ok"
    return _oracle[k]


def ceil64(n):
    return (int(n) + 63) // 64 * 64


def same_counts(o, r):
    for k in KEYS:
        assert o[k] == r[k], k


@pytest.mark.parametrize("key", list(EXACT))
def test_a_dense_table_that_fits_exactly(amd, key):
    spec, params = case = EXACT[key]
    o = oracle_of(case)
    cap = ceil64(o["distinct"])
    load = o["distinct"] / cap
    print(key, "distinct", o["distinct"], "table", cap, "load", load)
    assert cap <= 2048 * 8 and load >= (0.99 if key == "raft" else 0.95)
    eng = amd.Engine(spec, params, table_capacity=cap, arena_capacity=1 << 16, chunk_states=CHUNK, trace=False)
    try:
        assert eng.seen_layout() == (cap // 8, 8)   # the dense form
        same_counts(o, eng.run())
    finally:
        eng.close()
    # 64 slots fewer: fewer slots than states
    eng = amd.Engine(spec, params, table_capacity=cap - 64, arena_capacity=1 << 16, chunk_states=CHUNK, trace=False)
    try:
        assert eng.seen_layout() == (cap // 8 - 8, 8) and cap - 64 < o["distinct"]
        with pytest.raises(amd.McError) as e:
            eng.run()
        assert e.value.code == MC_ETABLEFULL
    finally:
        eng.close()


@pytest.mark.parametrize("key", list(LARGER))
def test_a_dense_table_at_load_nine_tenths(amd, key):
    spec, params = case = LARGER[key]
    o = oracle_of(case)
    cap = ceil64(o["distinct"] / 0.9)
    load = o["distinct"] / cap
    print(key, "distinct", o["distinct"], "table", cap, "load", load)
    assert 30000 <= o["distinct"] <= 300000 and 0.89 <= load <= 0.91
    eng = amd.Engine(spec, params, table_capacity=cap, arena_capacity=1 << 18, chunk_states=CHUNK, trace=False)
    try:
        assert eng.seen_layout() == (cap // 8, 8)
        same_counts(o, eng.run())
    finally:
        eng.close()


def test_the_sparse_form_at_load_four_fifths():
    """4-slot buckets — k_expand_pairs' pipelined prober, the by-family kernel's 4-slot probes — far above the third of a load they meet
    in any run that chose them by itself.  The appenders of engine_kernels.h and engine_pairs.h claim exactly the states they write
    (atomicAdd on arena_next by the survivors' count, refused when the end lies beyond arena_capacity), so the arena needs no slack beyond
    the states themselves; TLAMC_SPARSE_RATIO is read once per process: a child."""
    jobs, want = [], []
    for key in ("ssi", "raft"):
        spec, params = case = LARGER[key]
        o = oracle_of(case)
        arena = ceil64(o["distinct"]) + 64
        table = ceil64(1.25 * arena)
        assert o["distinct"] / table >= 0.7
        jobs.append(dict(spec=spec, params=params, kw=dict(table_capacity=table, arena_capacity=arena, chunk_states=CHUNK, trace=False)))
        want.append((o, table))
    env = dict(os.environ, TLAMC_SPARSE_RATIO="1.25")
    env.pop("TLAMC_DENSE_TABLE", None)
    p = subprocess.run([sys.executable, str(helpers.ROOT / "tests" / "seen_load_worker.py"), json.dumps(jobs)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    got = json.loads(next(line for line in p.stdout.splitlines() if line.startswith("RESULT "))[7:])
    for (o, table), r in zip(want, got):
        print(r.get("layout"), "distinct", o["distinct"], "load", o["distinct"] / table)
        assert "error" not in r, r
        assert r["layout"] == [table // 4, 4]   # the engine did choose the sparse form
        same_counts(o, r)


def test_the_state_graph_after_a_run_into_an_exactly_fitting_table(amd, tmp_path_factory):
    """seen_find on the device over long chains that wrap: every edge of the oracle's graph, by state text"""
    from test_gpu_graph import check_against_oracle, graph
    spec, params = case = EXACT["raft"]
    o = oracle_of(case)
    cap = ceil64(o["distinct"])
    assert o["distinct"] / cap >= 0.99
    g = graph(tmp_path_factory, spec, helpers.raft_oracle_params(params), True)
    eng = amd.Engine(spec, params, table_capacity=cap, arena_capacity=1 << 16, chunk_states=CHUNK)
    try:
        assert eng.seen_layout() == (cap // 8, 8)
        r = eng.run()
        same_counts(o, r)
        info, got, _, _ = check_against_oracle(g, eng, r, None)
        assert info.edges == sum(got.values()) > 0
    finally:
        eng.close()
