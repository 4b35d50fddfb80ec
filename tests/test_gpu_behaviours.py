"""Behaviour checking on the GPU (mc_engine_behaviours, k_behaviours in tla_rust_amd/csrc/engine_behaviours.h): the device's verdict
array is the host's (tests/_behshim: behaviour.h's beh_check over the same lowering) field for field — whatever the batch size, the
behaviours' lengths against `iters`, the batch's order or the engine's capacities — for the interpreter and for hand lowerings; recorded
simulation walks are behaviours of their model; what is refused is refused with a reason.  The kernel built over a test lowering
(tests/_behshim/behshim.hip) is the host rule too, and each of its three mutant builds fails the case made for the place it breaks.
`mc X.tla -behaviours FILE` on a file with a good and a bad behaviour: exit status, witness and wording."""
import random

import pytest

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


def walks(m, n, seed, lengths=LENGTHS, tamper=True):
    """n behaviours of the model: seeded random walks through the lowering's own successors, lengths in turn from `lengths`; every
    third one has an observation swapped for another walk's state (most of those are no behaviour)"""
    rng = random.Random(seed)
    inits, succ = m.inits(), {}
    out = []
    for k in range(n):
        rows = [rng.choice(inits)]
        while len(rows) < lengths[k % len(lengths)]:
            if rows[-1] not in succ:
                succ[rows[-1]] = [t for _, _, t in m.successors(rows[-1]) if t is not None]
            if not succ[rows[-1]]:
                break
            rows.append(rng.choice(succ[rows[-1]]))
        out.append(rows)
    if tamper:
        for k in range(2, n, 3):
            other = out[rng.randrange(n)]
            out[k] = list(out[k])
            out[k][rng.randrange(len(out[k]))] = other[rng.randrange(len(other))]
    return out


def device_is_host(amd, spec, params, m, batch, mask=None, stutter=False, iters=ITERS, caps=SMALL):
    eng = amd.Engine(spec, params, **caps)
    try:
        r = eng.behaviours(batch, mask=mask, stutter=stutter, iters=iters)
    finally:
        eng.close()
    want = m.check(batch, mask, stutter)
    assert [dict(v) for v in r.verdicts] == want
    kinds = [v["verdict"] for v in want]
    assert (r.accepted, r.rejected, r.ambiguous) == (kinds.count("accepted"), kinds.count("rejected"), kinds.count("ambiguous"))
    assert r.generated == sum(v["generated"] for v in want)
    assert r.observations == sum(len(b) if v["verdict"] == "accepted" else v["step"] + 1 for b, v in zip(batch, want))
    assert r.first_rejected == (kinds.index("rejected") if "rejected" in kinds else None)
    return r, want


@pytest.fixture(scope="module")
def peterson(amd):
    prog = host.program(*host.PROGRAMS["peterson"][:2])
    m = host.model("peterson")
    return prog, m, walks(m, 257, seed=1), prog.observe(["flag", "turn", "in_cs"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batches_of_every_size_with_pc_hidden(amd, peterson, n):
    prog, m, batch, mask = peterson
    r, want = device_is_host(amd, "pcal", prog.params, m, batch[:n], mask)
    if n == 257:
        assert {len(b) for b in batch} == set(LENGTHS) and r.rejected > 10 and r.accepted > 100 and max(v["peak"] for v in want) > 1


def test_full_mask_stutter_and_one_launch(amd, peterson):
    prog, m, batch, mask = peterson
    device_is_host(amd, "pcal", prog.params, m, batch[:100])
    device_is_host(amd, "pcal", prog.params, m, batch[:100], mask, stutter=True)
    device_is_host(amd, "pcal", prog.params, m, batch[:100], mask, iters=0, caps=dict(SMALL, chunk_states=1 << 16))   # the default: one launch, one round


def test_a_permuted_batch_gives_the_permuted_verdicts(amd, peterson):
    prog, m, batch, mask = peterson
    order = list(range(200))
    random.Random(5).shuffle(order)
    eng = amd.Engine("pcal", prog.params, **SMALL)
    a = eng.behaviours(batch[:200], mask=mask, iters=ITERS).verdicts
    b = eng.behaviours([batch[k] for k in order], mask=mask, iters=ITERS).verdicts
    eng.close()
    assert b == [a[k] for k in order]


def test_the_models_of_specs_behaviours(amd):
    """tests/test_behaviours_host.py's named cases, on the device: full candidate sets, lane pairs that bring one row in one round,
    AMBIGUOUS at observation 0 and later, converging candidates, steps outside a CONSTRAINT, a failing Assert, rows that share a
    VIEW fingerprint"""
    want = host.named_cases()
    for name, (params, batch, mask, stutter) in host.case_inputs().items():
        eng = amd.Engine("pcal", params, **SMALL)
        got = eng.behaviours(batch, mask=mask, stutter=stutter, iters=ITERS).verdicts
        eng.close()
        assert [dict(v) for v in got] == want[name], name
        assert name not in host.EXPECTED or want[name] == host.EXPECTED[name]


# ------------------------------------------------------------------------------------------------ the kernel against its mutants
FULL = (1 << 64) - 1


def hide_cases():
    """{case: (K, B, batch of (x, h) rows, mask)} over behshim.hip's lowering SpecHide, each made for one place of the kernel"""
    x_only = (FULL, 0)
    return {
        # 64 members fold pairwise onto 32 rows: lanes 2j and 2j + 1 bring the same row in the same round
        "dedup across the lanes of one round": (64, 0, [[(0, 0), (1, 0), (2, 0)], [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0)]], x_only),
        # h is observed through the low half of the LAST mask word (not a full mask: no fingerprint shortcut): one candidate
        "the last word of the mask": (64, 0, [[(0, 5), (1, 2), (2, 1)], [(0, 63)], [(0, 7), (1, 4)]], (FULL, 0xffffffff)),
        # 65 initial states, and 40 members with 1 + 2 successors each: more than 64 rows at observation 0 / 1
        "lane 64 and beyond": (40, 2, [[(0, 0), (1, 0)], [(0, 0), (1, 0), (2, 0), (3, 0)]], x_only),
        "lane 64 and beyond among the initial states": (65, 0, [[(0, 0), (1, 0)]], x_only),
    }


MUTANT_CASE = {1: ["dedup across the lanes of one round"], 2: ["the last word of the mask"],
               3: ["lane 64 and beyond", "lane 64 and beyond among the initial states"]}


def test_the_kernel_over_the_test_lowering_is_the_host_rule(amd):
    hm = behshim.HideModel(0)
    got = {name: (hm.device(K, B, batch, mask), hm.host(K, B, batch, mask)) for name, (K, B, batch, mask) in hide_cases().items()}
    for name, (dev, want) in got.items():
        assert dev == want, name
    v = host.v
    assert got["dedup across the lanes of one round"][1] == [v("accepted", 3, 16, 64, 64 + 64 + 32), v("accepted", 7, 1, 64, 64 + 64 + 32 + 16 + 8 + 4 + 2)]
    assert got["the last word of the mask"][1] == [v("accepted", 3, 1, 1, 64 + 1 + 1), v("accepted", 1, 1, 1, 64), v("rejected", 1, 1, 1, 64 + 1)]
    assert got["lane 64 and beyond"][1] == [v("ambiguous", 1, 40, 40, 40 + 120)] * 2
    assert got["lane 64 and beyond among the initial states"][1] == [v("ambiguous", 0, 0, 0, 65)]


@pytest.mark.parametrize("mutant", [1, 2, 3])
def test_a_broken_kernel_is_told_from_the_product(amd, mutant):
    """the kernel with one thing broken (behshim.hip, -DBEH_MUTANT=n) fails the case made for that place: these cases do look there"""
    hm = behshim.HideModel(mutant)
    for name in MUTANT_CASE[mutant]:
        K, B, batch, mask = hide_cases()[name]
        assert hm.device(K, B, batch, mask) != hm.host(K, B, batch, mask), name


# ------------------------------------------------------------------------------------------------ the command
LOG = """State 1: <Initial predicate>
/\\ x = 0

State 2: <Action s of module diamond>
/\\ x = 1
--------
/\\ x = 0

/\\ x = 0
"""


def run_mc(*args):
    import subprocess
    p = subprocess.run([str(ROOT / "tla_rust_amd" / "_build" / "mc"), *map(str, args)], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout, p.stderr


def test_cli_one_good_and_one_bad_behaviour(tmp_path):
    log = tmp_path / "log.txt"
    log.write_text(LOG)
    tla = ROOT / "specs_behaviours" / "diamond.tla"
    rc, out, err = run_mc(tla, "-behaviours", log)   # (no -observe: x is what every state of the file mentions)
    assert rc == 12, (out, err)
    assert "Error: Behaviour 2 is not a behaviour of the model: no step leads to observation 2.\n" in out
    # the witness: one model path up to the observation, in TLC's layout; then the observation itself
    assert "Error: The behavior of the model up to this point is:\nState 1: <Initial predicate>\n/\\ h = 1\n/\\ x = 0\n/\\ pc = (0 :> \"s\")\n\n" in out
    assert "State 2:" not in out and "The observation is:\n/\\ x = 0\n" in out
    assert "2 behaviours checked: 1 accepted, 1 rejected, 0 ambiguous.\n" in out and "Warning" not in out
    assert run_mc(tla, "-behaviours", log, "-observe", "x")[:2] == (rc, out)
    rc, out, err = run_mc(tla, "-behaviours", log, "-stutter")
    assert rc == 0 and "2 behaviours checked: 2 accepted, 0 rejected, 0 ambiguous.\n" in out and "Error" not in out, (out, err)
    # a rejected behaviour with a step before it: the witness names the action
    log.write_text("/\\ x = 0\n\n/\\ x = 1\n\n/\\ x = 0\n")
    rc, out, err = run_mc(tla, "-behaviours", log)
    assert rc == 12 and "no step leads to observation 3." in out and "State 2: <Action s of module diamond>\n/\\ h = 0\n/\\ x = 1\n" in out, (out, err)
    # ambiguous behaviours are named in a warning and counted; exit status 0
    log.write_text("/\\ x = 0\n")
    rc, out, err = run_mc(ROOT / "specs_behaviours" / "hidden_choice.tla", "-config", ROOT / "specs_behaviours" / "hidden_choice_65.cfg", "-behaviours", log)
    assert rc == 0 and "Warning: 1 behaviours are ambiguous" in out and ": 1 (at observation 1)\n" in out and "0 accepted, 0 rejected, 1 ambiguous" in out, (out, err)
    rc, out, err = run_mc(tla, "-behaviours", log, "-observe", "h")
    assert rc == 1 and "does not mention every variable of -observe h" in err
    log.write_text("/\\ y = 0\n")
    rc, out, err = run_mc(tla, "-behaviours", log)
    assert rc == 1 and "no variable `y`" in err


HAND = [("atomic_add", [3]), ("raft", [2, 2, 2, 9, 1, 1]), ("ssi", [2, 1, 127, 0])]


@pytest.mark.parametrize("spec,params", HAND, ids=[s for s, _ in HAND])
def test_hand_lowerings(amd, spec, params):
    m = behshim.Model(spec, params)
    device_is_host(amd, spec, params, m, walks(m, 130, seed=3, lengths=(1, 2, 3, 4, 7, 12)))


SIMULATED = [("atomic_add", [10]), ("raft", [2, 2, 2, 9, 1, 1])]   # (atomic_add with 10 adders: walks of 12 states, more than two launches)


@pytest.mark.parametrize("spec,params", SIMULATED, ids=[s for s, _ in SIMULATED])
def test_recorded_simulation_walks_are_behaviours(amd, spec, params):
    m = behshim.Model(spec, params)
    (init,) = m.inits()   # (one initial state: a walk's first state needs no hash)
    eng = amd.Engine(spec, params, **SMALL)
    sim = eng.simulate(64, 20, 7, record=64)
    batch = []
    for w in sim.recorded:
        rows = [init]
        for slot in w["slots"]:
            rows.append(amd.binding.state_apply(spec, params, rows[-1], slot))
        assert len(rows) == w["len"]
        batch.append(rows)
    r = eng.behaviours(batch, iters=ITERS)
    eng.close()
    assert r.accepted == 64 and all(v.candidates == 1 and v.step == len(b) for v, b in zip(r.verdicts, batch))
    assert max(map(len, batch)) > 2 * ITERS


def test_the_witness_is_the_hosts(amd, peterson):
    prog, m, batch, mask = peterson
    eng = amd.Engine("pcal", prog.params, **SMALL)
    try:
        r = eng.behaviours(batch[:60], mask=mask, iters=ITERS)
        for b, v in enumerate(r.verdicts):
            wit = eng.behaviour_witness(batch[:60], b, mask=mask)
            assert wit == m.sets(batch[b], mask)[2] and len(wit) == v.step
    finally:
        eng.close()


MANY = """---- MODULE many ----
EXTENDS Naturals
(* --algorithm many
variables a \\in 1..300, b \\in 1..300;
process P = 0
begin
  s: a := b;
end process
end algorithm *)
====
"""


def test_refusals(amd, peterson):
    prog, m, batch, mask = peterson
    eng = amd.Engine("pcal", prog.params, **SMALL)
    with pytest.raises(amd.McError, match="is empty") as e:
        eng.behaviours([batch[0], []])
    assert e.value.code == -1
    eng.close()
    many = amd.Program(MANY, "SPECIFICATION Spec\n")   # 300 * 300 initial states
    eng = amd.Engine("pcal", many.params, **SMALL)
    with pytest.raises(amd.McError, match="more than 65536 initial states"):
        eng.behaviours([[bytes(16)]])
    eng.close()
    many.close()
    eng = amd.Engine("atomic_add", [3], shard_rank=0, shard_count=2, **SMALL)
    with pytest.raises(amd.McError, match="sharded"):
        eng.behaviours([[bytes(8)]])
    eng.close()


def test_a_generated_code_engine_is_refused(amd, peterson):
    prog, m, batch, mask = peterson
    eng = amd.Engine("pcal", prog.params, jit=True, **SMALL)
    with pytest.raises(amd.McError, match="MC_F_JIT.*packs its rows.*import_row") as e:
        eng.behaviours(batch[:2])
    assert e.value.code == -1
    eng.close()
