"""Behaviour checking with unlogged steps on the GPU (MC_BEH_F_HIDDEN: k_behaviours<S, 0, true> in tla_rust_amd/csrc/engine_behaviours.h).
Through the engine the device's verdict array is the host rule's (behaviour.h's beh_check with g++, held against a plain reference in
tests/test_behaviours_hidden_host.py) field for field: peterson logged without pc at H = 1, 2, 5, with and without stuttering, batches
of 1, 64, 65 and 257, a permuted batch; the raft hand lowering with one server's word hidden; the path with the hidden states in it;
`mc -behaviours FILE -hidden H`.  The kernel over the test lowering SpecGap (tests/_behshim/behgap.hip) gives the figures worked out by
hand for each place the closure can go wrong, and each of its three mutant builds fails the case made for it."""
import random

import pytest

import behgap
import behshim
import helpers
import test_behaviours_host as host

pytestmark = pytest.mark.gpu
ROOT = helpers.ROOT
SMALL = dict(table_capacity=1 << 16, arena_capacity=1 << 14, chunk_states=1 << 12)   # rounds of 64 behaviours
ITERS = 3
LENGTHS = (1, 2, 3, 4, 7)   # iters - 2, iters - 1, iters, iters + 1, 2 * iters + 1


@pytest.fixture(scope="module")
def amd():
    import tla_rust_amd
    assert tla_rust_amd.device_count() >= 1, "no HIP device visible"
    return tla_rust_amd


def logs(m, mask, n, seed, lengths=LENGTHS, tamper=True):
    """n logs of the model as an implementation would write them: seeded random walks through the lowering's own successors, a state
    kept when a cell under the mask differs from the last one kept, until the log has its length (in turn from `lengths`); every third
    log has an observation swapped for another log's (most of those are no behaviour)"""
    rng = random.Random(seed)
    inits, succ = m.inits(), {}

    def seen(row):
        return bytes(a & b for a, b in zip(row, mask))
    out = []
    for k in range(n):
        row = rng.choice(inits)
        kept = [row]
        for _ in range(80):
            if len(kept) == lengths[k % len(lengths)]:
                break
            if row not in succ:
                succ[row] = [t for _, _, t in m.successors(row) if t is not None]
            if not succ[row]:
                break
            row = rng.choice(succ[row])
            if seen(row) != seen(kept[-1]):
                kept.append(row)
        out.append(kept)
    if tamper:
        for k in range(2, n, 3):
            other = out[rng.randrange(n)]
            out[k] = list(out[k])
            out[k][rng.randrange(len(out[k]))] = other[rng.randrange(len(other))]
    return out


def device_is_host(eng, m, batch, mask, stutter, hidden, iters=ITERS):
    r = eng.behaviours(batch, mask=mask, stutter=stutter, iters=iters, hidden=hidden)
    want = behgap.hidden_check(m, batch, mask, stutter, hidden)
    assert [dict(v) for v in r.verdicts] == want, (stutter, hidden)
    kinds = [v["verdict"] for v in want]
    assert (r.accepted, r.rejected, r.ambiguous) == (kinds.count("accepted"), kinds.count("rejected"), kinds.count("ambiguous"))
    assert r.generated == sum(v["generated"] for v in want)
    assert r.first_rejected == (kinds.index("rejected") if "rejected" in kinds else None)
    return r, want


@pytest.fixture(scope="module")
def peterson(amd):
    prog = host.program(*host.PROGRAMS["peterson"][:2])
    m = host.model("peterson")
    mask = prog.observe(["flag", "turn", "in_cs"])
    return prog, m, logs(m, mask, 257, seed=1), mask


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_batches_of_every_size_with_pc_hidden(amd, peterson, n):
    prog, m, batch, mask = peterson
    eng = amd.Engine("pcal", prog.params, **SMALL)
    try:
        for hidden in (1, 2, 5):
            for stutter in (False, True):
                r, want = device_is_host(eng, m, batch[:n], mask, stutter, hidden)
                if n == 257 and not stutter:
                    assert {len(b) for b in batch} == set(LENGTHS) and r.rejected > 10 and r.accepted > 100 and r.ambiguous < 26
                    assert max(v["peak"] for v in want) > 2   # (closures wider than two lanes)
        # the bound matters: what H = 5 accepts, the plain rule rejects
        if n == 257:
            plain = eng.behaviours(batch, mask=mask, iters=ITERS)
            assert [dict(v) for v in plain.verdicts] == m.check(batch, mask) and plain.accepted < r.accepted
    finally:
        eng.close()


def test_a_permuted_batch_gives_the_permuted_verdicts(amd, peterson):
    prog, m, batch, mask = peterson
    order = list(range(200))
    random.Random(5).shuffle(order)
    eng = amd.Engine("pcal", prog.params, **SMALL)
    a = eng.behaviours(batch[:200], mask=mask, iters=ITERS, hidden=2).verdicts
    b = eng.behaviours([batch[k] for k in order], mask=mask, iters=ITERS, hidden=2).verdicts
    eng.close()
    assert b == [a[k] for k in order]


def test_the_raft_hand_lowering(amd):
    """the engine stores raft rows in 13 words: the observations and the mask go through import_row.  Hidden: the fingerprint word and
    server 0's word — the steps that move only server 0 are not logged"""
    spec, params = "raft", [2, 2, 2, 9, 1, 1]
    m = behshim.Model(spec, params)
    mask = bytearray(b"\xff" * m.W)
    for word in (0, 2):
        mask[8 * word:8 * word + 8] = bytes(8)
    mask = bytes(mask)
    batch = logs(m, mask, 130, seed=3)
    eng = amd.Engine(spec, params, **SMALL)
    try:
        r, want = device_is_host(eng, m, batch, mask, False, 1)
        assert r.accepted > 40 and max(v["peak"] for v in want) > 1
        plain = eng.behaviours(batch, mask=mask, iters=ITERS)
        assert plain.accepted < r.accepted
    finally:
        eng.close()


def test_the_path_is_the_hosts(amd, peterson):
    prog, m, batch, mask = peterson
    eng = amd.Engine("pcal", prog.params, **SMALL)
    try:
        r = eng.behaviours(batch[:40], mask=mask, iters=ITERS, hidden=2)
        hidden_states = 0
        for b, v in enumerate(r.verdicts):
            path = eng.behaviour_path(batch[:40], b, mask=mask, hidden=2)
            assert path == behgap.hidden_path(m, batch[b], mask, hidden=2)[1]
            assert sorted({at for _, _, at in path}) == list(range(v.step)) and len(path) <= 3 * max(v.step, 1)
            hidden_states += len(path) - v.step
        assert hidden_states > 10
        assert eng.behaviour_path(batch[:40], 0, mask=mask) == [(s, row, k) for k, (s, row) in enumerate(eng.behaviour_witness(batch[:40], 0, mask=mask))]
        with pytest.raises(amd.McError, match="mc_engine_behaviour_path") as e:
            eng.behaviour_witness(batch[:40], 0, mask=mask, hidden=2)
        assert e.value.code == -1
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ the kernel over SpecGap
def test_the_kernel_over_the_test_lowering_is_the_host_rule(amd):
    gm = behgap.GapModel(0)
    for name, (case, batch, hidden, iters, want) in behgap.GAP_CASES.items():
        assert gm.host(case, batch, behgap.X_ONLY, hidden=hidden) == want, name
        assert gm.device(case, batch, behgap.X_ONLY, hidden=hidden, iters=iters) == want, name
    # the cases in one batch, stuttering allowed (x = 0, 0 may then be one state twice), and one launch for everything
    case, batch = (1, 0, 2, 0, 0), [behgap.xs(0, 0, 1), behgap.xs(0, 1, 1, 2), behgap.xs(0, 0, 0, 0, 1), behgap.xs(0, 2)]
    for iters in (3, 16):
        assert gm.device(case, batch, behgap.X_ONLY, True, 2, iters) == gm.host(case, batch, behgap.X_ONLY, True, 2)


@pytest.mark.parametrize("mutant", [4, 5, 6])
def test_a_broken_kernel_is_told_from_the_product(amd, mutant):
    """the kernel with one thing broken (behgap.hip, -DBEH_MUTANT=n) fails the case made for that place; every mutant still stays inside
    its 64 columns and its H + 1 depths"""
    gm = behgap.GapModel(mutant)
    case, batch, hidden, iters, want = behgap.GAP_CASES[behgap.MUTANT_CASE[mutant]]
    assert gm.device(case, batch, behgap.X_ONLY, hidden=hidden, iters=iters) != want


# ------------------------------------------------------------------------------------------------ the command
def run_mc(*args):
    import subprocess
    p = subprocess.run([str(ROOT / "tla_rust_amd" / "_build" / "mc"), *map(str, args)], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout, p.stderr


def test_cli_hidden(tmp_path):
    log = tmp_path / "log.txt"
    log.write_text("/\\ x = 0\n\n/\\ x = 1\n\n/\\ x = 3\n")
    tla, leaky = ROOT / "specs_behaviours" / "unlogged.tla", ROOT / "specs_behaviours" / "unlogged_leaky.cfg"
    rc, out, err = run_mc(tla, "-behaviours", log)
    assert rc == 12 and "no step leads to observation 3.\n" in out, (out, err)
    rc, out, err = run_mc(tla, "-behaviours", log, "-hidden", 1)
    assert rc == 12 and "no step, and no step after up to 1 unlogged ones, leads to observation 3.\n" in out, (out, err)
    assert ", up to 1 unlogged steps between observations.\n" in out
    rc, out, err = run_mc(tla, "-behaviours", log, "-hidden", 2)
    assert rc == 0 and "1 behaviours checked: 1 accepted, 0 rejected, 0 ambiguous.\n" in out and "Error" not in out, (out, err)
    assert "up to 2 unlogged steps between observations" in out
    rc, out, err = run_mc(tla, "-config", leaky, "-behaviours", log, "-hidden", 2)
    assert rc == 12 and "leads to observation 3.\n" in out, (out, err)
    # a rejected log with unlogged steps before the observation nothing leads to: the witness shows them
    log.write_text("/\\ x = 0\n\n/\\ x = 1\n\n/\\ x = 3\n\n/\\ x = 4\n")
    rc, out, err = run_mc(tla, "-behaviours", log, "-hidden", 2)
    assert rc == 12 and "leads to observation 4.\n" in out, (out, err)
    assert "State 2: <Action a of module unlogged>\n" in out and "State 3: <Action b of module unlogged> (not logged)\n" in out
    assert "State 4: <Action c of module unlogged> (not logged)\n" in out and "State 5: <Action d of module unlogged>\n" in out
