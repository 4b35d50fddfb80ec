"""Raft on one GPU stores its rows in fewer words (tla_rust_amd/csrc/spec_raft_packed.h; $TLAMC_RAFT_PACK=0: the rows of every other
engine).  Both engines must find the same states — per-level counts equal to the oracle's goldens, the same rows out of
mc_engine_read_states, the same counterexample — and everything that leaves the engine keeps the public width (mc_state_bytes)."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "raft_levels.json"
K5 = [3, 4, 2, 3, 1, 1, 10, 1, 4, 5]   # raft3_mcr4_t2_m1_k5_complete in the capacities of the bench rows: 16 words, 13 packed
MC_EBADCFG = -1


@pytest.fixture(scope="module")
def amd():
    import tla_rust_amd
    assert tla_rust_amd.device_count() >= 1, "no HIP device visible"
    return tla_rust_amd


def golden(name):
    return next(c for c in json.loads(GOLDEN.read_text())["cases"] if c["name"] == name)


def engine(amd, monkeypatch, packed, params, **kw):
    """the environment is read when the engine is created"""
    if packed:
        monkeypatch.delenv("TLAMC_RAFT_PACK", raising=False)
    else:
        monkeypatch.setenv("TLAMC_RAFT_PACK", "0")
    return amd.Engine("raft", params, **kw)


def canonical(params, rows):
    """rows (n x words, uint64, public layout) with every slot array in order.

    messages, elections and allLogs are UNORDERED slot arrays (spec_raft.h: the fingerprint is a multiset sum): one TLA+ state has
    several rows, and which of them is stored depends on which parent's wavefront won the insert — two runs of the SAME engine
    differ in the message words of more than half of the 178 654 rows of the k5 graph.  Equal states are equal rows once every
    slot array is sorted, which is all this does to a row."""
    p = list(params) + [0] * 9
    ns, cm, ce, ca = p[0], p[6] or 40, p[7] or 4, p[8] or 16
    m0, e0 = 2 + 2 * ns, 2 + 2 * ns + (cm + 1) // 2
    a0 = e0 + 2 * ce
    assert a0 + (ca + 3) // 4 == rows.shape[1]
    rows[:, m0:e0] = np.sort(np.ascontiguousarray(rows[:, m0:e0]).view(np.uint32), axis=1).view(np.uint64)
    rows[:, a0:] = np.sort(np.ascontiguousarray(rows[:, a0:]).view(np.uint16), axis=1).view(np.uint64)
    for k in range(ce - 1, 0, -1):   # election records (two words each) by (word 0, word 1): a bubble pass per record
        for j in range(k):
            x, y = e0 + 2 * j, e0 + 2 * j + 2
            swap = (rows[:, x] > rows[:, y]) | ((rows[:, x] == rows[:, y]) & (rows[:, x + 1] > rows[:, y + 1]))
            rows[swap, x:y + 2] = rows[swap][:, [y, y + 1, x, x + 1]]
    return rows


def rows_by_fingerprint(amd, eng, n):
    """every stored row in the public layout, canonical, ordered by its fingerprint (word 0: unique per state)"""
    W = amd.state_bytes("raft", eng.params)
    buf = np.empty(n * W, dtype=np.uint8)
    rc = amd.lib().mc_engine_read_states(eng._h, 0, n, C.c_void_p(buf.ctypes.data))
    assert rc == 0, amd.lib().mc_last_error()
    rows = canonical(eng.params, buf.view(np.uint64).reshape(n, W // 8))
    return rows[np.argsort(rows[:, 0], kind="stable")]


@pytest.mark.parametrize("name,caps", [("raft3_mcr4_t2_m1_k5_complete", (10, 1, 4)), ("raft2_mcr1_t3_m1", (22, 2, 4))])
def test_both_row_widths_find_the_same_states(amd, oracle, monkeypatch, name, caps):
    c = golden(name)
    params = oracle.raft_device_params(c["params"], *caps)
    out = {}
    for packed in (True, False):
        eng = engine(amd, monkeypatch, packed, params, table_capacity=4 * c["distinct"], arena_capacity=c["distinct"] + (1 << 16),
                     chunk_states=1 << 19, trace=False)
        r = eng.run()
        assert r.levels == c["levels"]
        assert (r.distinct, r.generated, r.depth, r.verdict, r.queue_left) == (c["distinct"], c["generated"], c["depth"], "ok", 0)
        out[packed] = (eng.kernel_stats()["state_bytes"], rows_by_fingerprint(amd, eng, r.distinct))
        eng.close()
    assert out[True][0] < out[False][0] == amd.state_bytes("raft", params)
    assert len(np.unique(out[True][1][:, 0])) == c["distinct"]
    assert np.array_equal(out[True][1], out[False][1])


def test_stored_row_width(amd, monkeypatch):
    assert amd.state_bytes("raft", K5) == 128
    for packed, want in ((True, 104), (False, 128)):
        eng = engine(amd, monkeypatch, packed, K5, table_capacity=1 << 20, arena_capacity=1 << 18, chunk_states=1 << 12, max_levels=3)
        eng.run()
        assert eng.kernel_stats()["state_bytes"] == want
        assert all(len(s) == 128 for s in eng.read_states(0, 4))
        eng.close()


def raw_trace(amd, eng):
    W = amd.state_bytes("raft", eng.params)
    cap = C.c_size_t(4096)
    states = C.create_string_buffer(W * cap.value)
    acts = (C.c_int32 * cap.value)()
    assert amd.lib().mc_engine_trace(eng._h, states, acts, C.byref(cap)) == 0
    return states.raw[:W * cap.value], list(acts[:cap.value])


def test_a_violation_gives_the_same_trace(amd, monkeypatch):
    """CommittedLogStable is violated at MaxTerm = 3, MaxClientRequests = 3 (tests/test_gpu_parity.py): 31 states.  Which shortest
    counterexample an engine reports depends on which parent stored a state first (any engine, run to run), so "the same trace" is:
    the same verdict, invariant, length and depth, the same first state and last action, and a trace that the HOST lowering of
    the public rows (mc_state_apply: spec_raft.h, never the packed class) accepts step by step from Init."""
    params = [2, 3, 3, 9, 1, 2]
    W = amd.state_bytes("raft", params)
    nslots = 5 * 2 + 2 * 4 + 3 * 40
    out = {}
    for packed in (True, False):
        eng = engine(amd, monkeypatch, packed, params, table_capacity=1 << 26, arena_capacity=1 << 25, chunk_states=1 << 18)
        r = eng.run()
        assert (r.verdict, r.violated_invariant, r.trace_len) == ("invariant", 1, 31)
        (states, acts), text = raw_trace(amd, eng), eng.trace()
        eng.close()
        assert len(states) == 31 * W and len(text) == 31
        rows = [states[k * W:(k + 1) * W] for k in range(31)]
        canon = lambda b: canonical(params, np.frombuffer(b, dtype=np.uint64).reshape(1, W // 8).copy()).tobytes()
        for k in range(30):
            want = canon(rows[k + 1])
            slots = [s for s in range(nslots) if canon(amd.binding.state_apply("raft", params, rows[k], s)) == want]
            assert slots, k
            assert text[k + 1][0] in {amd.binding.state_action_name("raft", params, rows[k], s) for s in slots}, k
        out[packed] = (rows[0], text[0], text[-1][0], acts[0], acts[-1], r.depth)
    assert out[True] == out[False]
    assert out[True][2] == "AdvanceCommitIndex"


def test_checkpoint_round_trip_and_the_other_width_refused(amd, monkeypatch, tmp_path):
    c = golden("raft3_mcr4_t2_m1_k5_complete")
    kw = dict(table_capacity=1 << 20, arena_capacity=1 << 18, chunk_states=1 << 12)
    files = {}
    for packed in (True, False):
        a = engine(amd, monkeypatch, packed, K5, max_levels=9, **kw)
        ra = a.run()
        assert ra.verdict == "budget" and ra.levels == c["levels"][:9]
        files[packed] = tmp_path / f"k5_{int(packed)}.ck"
        a.checkpoint(files[packed])
        a.close()
    assert files[True].stat().st_size < files[False].stat().st_size
    for packed in (True, False):
        b = engine(amd, monkeypatch, packed, K5, **kw)
        b.restore(files[packed])
        rb = b.run()
        assert (rb.levels, rb.distinct, rb.generated, rb.verdict) == (c["levels"], c["distinct"], c["generated"], "ok")
        b.close()
        other = engine(amd, monkeypatch, packed, K5, **kw)
        with pytest.raises(amd.McError) as ei:      # rows of the other width are refused by the header's word count, never read
            other.restore(files[not packed])
        assert ei.value.code == MC_EBADCFG
        assert other.run().distinct == c["distinct"]   # ... and the engine is as it was
        other.close()


def test_shard_calls_on_a_one_gpu_engine(amd, monkeypatch):
    """the step calls exchange public rows: an engine that has not searched is made again unpacked behind its handle, one that has refuses"""
    kw = dict(table_capacity=1 << 20, arena_capacity=1 << 18, chunk_states=1 << 12)
    eng = engine(amd, monkeypatch, True, K5, **kw)
    eng.shard_begin()
    assert eng.shard_level_size() == 1 and eng.kernel_stats()["state_bytes"] == 128
    eng.close()
    eng = engine(amd, monkeypatch, True, K5, max_levels=3, **kw)
    eng.run()
    with pytest.raises(amd.McError) as ei:
        eng.shard_begin()
    assert ei.value.code == MC_EBADCFG and "TLAMC_RAFT_PACK" in str(ei.value)
    assert eng.kernel_stats()["state_bytes"] == 104
    eng.close()
