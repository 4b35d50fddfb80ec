"""Behaviour checking with unlogged steps (MC_BEH_F_HIDDEN) on the host: behaviour.h's beh_check, built with g++ (tests/_behshim), against
a plain restatement of the rule over the oracle's state graph (tests/behaviours_hidden.py).  peterson logged as an implementation
would — flag, turn and in_cs when one of them changes, never pc — is accepted at H = the longest run of steps the log dropped and
rejected one step short; H = 0 is the flag-less call and a full mask makes H irrelevant; a larger H never turns accepted into
rejected; the path with the hidden states in it is a path of the graph; the cases of the test lowering (tests/behgap.py) give the
figures worked out by hand; seven one-line mutants of behaviour.h each fail a named case.  Nothing here needs a GPU."""
import random
import subprocess
from functools import lru_cache

import pytest

import behaviours
import behaviours_hidden as bh
import behgap
import behshim
import helpers
import test_behaviours_host as host
import testlib

ROOT = helpers.ROOT
SB = ROOT / "specs_behaviours"
OBSERVED = ["flag", "in_cs", "turn"]   # what an implementation of peterson can see; pc is the model's
WALKS, WALK_LEN, SEED = 120, 14, 11


def kept_indices(texts, names):
    """the states of a walk a log keeps that records only when an observed variable changes, and the longest run it drops between two"""
    kept, longest = [0], 0
    for k in range(1, len(texts)):
        if behaviours.observe(texts[k], names) != behaviours.observe(texts[kept[-1]], names):
            longest = max(longest, k - kept[-1] - 1)
            kept.append(k)
    return kept, longest


@lru_cache(maxsize=None)
def peterson_logs():
    """[(texts of the walk, indices kept, longest dropped run)]: seeded walks of the graph from its initial state"""
    g = host.graph("peterson")
    rng = random.Random(SEED)
    out = []
    for k in range(WALKS):
        texts = [g.init[0].text]
        while len(texts) < 4 + k % (WALK_LEN - 3):
            texts.append(rng.choice([e.text for e in g.succ[texts[-1]] if not e.flags]))
        kept, longest = kept_indices(texts, OBSERVED)
        out.append((tuple(texts), tuple(kept), longest))
    return out


@lru_cache(maxsize=None)
def peterson_inputs():
    """(model, mask, [rows of each log], [observations of each log])"""
    m, rows = host.model("peterson"), host.rows_of("peterson")
    mask = host.program(*host.PROGRAMS["peterson"][:2]).observe(OBSERVED)
    batch, obs = [], []
    for texts, kept, _ in peterson_logs():
        r = rows.of_path(texts)
        batch.append([r[k] for k in kept])
        obs.append([behaviours.observe(texts[k], OBSERVED) for k in kept])
    return m, mask, batch, obs


@lru_cache(maxsize=None)
def reference(hidden_of, stutter=False):
    """the Python rule's verdict of every log at H = hidden_of(longest dropped run); hidden_of: "longest", "short" (one less) or a number"""
    g = host.graph("peterson")
    _, _, _, obs = peterson_inputs()
    out = []
    for (_, _, longest), o in zip(peterson_logs(), obs):
        h = longest if hidden_of == "longest" else max(longest - 1, 0) if hidden_of == "short" else hidden_of
        out.append(bh.check(g, o, OBSERVED, stutter, h)[0])
    return out


def host_verdicts(hidden_of, stutter=False):
    """the same from behaviour.h: one call per H (a batch has one H)"""
    m, mask, batch, _ = peterson_inputs()
    logs = peterson_logs()
    hs = [lg[2] if hidden_of == "longest" else max(lg[2] - 1, 0) if hidden_of == "short" else hidden_of for lg in logs]
    out = [None] * len(batch)
    for h in sorted(set(hs)):
        idx = [k for k, x in enumerate(hs) if x == h]
        for k, v in zip(idx, behgap.hidden_check(m, [batch[k] for k in idx], mask, stutter, h)):
            out[k] = v
    return out


def test_compressed_logs_are_accepted_at_their_longest_dropped_run():
    want = reference("longest")
    got = host_verdicts("longest")
    assert got == want
    assert all(v["verdict"] == "accepted" and v["step"] == len(lg[1]) for v, lg in zip(got, peterson_logs()))
    assert max(lg[2] for lg in peterson_logs()) >= 3 and max(v["peak"] for v in got) > 2   # (runs of several steps, sets wider than two)
    assert host_verdicts("longest", True) == reference("longest", True)


def test_one_step_short_is_rejected():
    want = reference("short")
    got = host_verdicts("short")
    assert got == want
    # walks whose longest dropped run has no shorter route: by the Python rule alone
    short = [k for k, (lg, v) in enumerate(zip(peterson_logs(), want)) if lg[2] >= 1 and v["verdict"] == "rejected"]
    assert len(short) >= 5, len(short)
    assert all(got[k]["verdict"] == "rejected" for k in short)


def test_the_inputs_decide():
    """under the Python rule alone at most 10 % of the verdicts these tests look at are ambiguous and at least half are accepted:
    `ambiguous` hides no failure here"""
    verdicts = [v["verdict"] for how in ("longest", "short", 0, 1, 2, 5) for v in reference(how)]
    assert verdicts.count("ambiguous") <= len(verdicts) // 10, verdicts.count("ambiguous")
    assert verdicts.count("accepted") >= len(verdicts) // 2, verdicts.count("accepted")


@pytest.mark.parametrize("hidden", [1, 2, 5])
def test_a_fixed_bound_is_the_references(hidden):
    assert host_verdicts(hidden) == reference(hidden)
    assert host_verdicts(hidden, True) == reference(hidden, True)


def test_no_hidden_steps_is_the_flagless_call_and_a_full_mask_makes_them_irrelevant():
    m, mask, batch, _ = peterson_inputs()
    assert behgap.hidden_check(m, batch, mask, hidden=0) == m.check(batch, mask) == reference(0)
    assert behgap.hidden_check(m, batch, mask, True, 0) == m.check(batch, mask, True)
    rows = host.rows_of("peterson")
    whole = [rows.of_path(lg[0]) for lg in peterson_logs()]   # every state logged, all of it
    assert behgap.hidden_check(m, whole, None, hidden=3) == m.check(whole)
    assert behgap.hidden_check(m, batch, None, hidden=3) == m.check(batch)   # (the compressed logs: mostly rejected, the same)


def test_a_larger_bound_never_rejects_what_a_smaller_one_accepts():
    per_h = [host_verdicts(h) for h in range(0, 7)]
    flips = 0
    for a, b in zip(per_h, per_h[1:]):
        for va, vb in zip(a, b):
            assert va["verdict"] != "accepted" or vb["verdict"] in ("accepted", "ambiguous")
            flips += va["verdict"] == "rejected" and vb["verdict"] == "accepted"
    assert flips > 10   # (the bound matters on these logs)


def test_the_path_is_a_path_of_the_graph():
    g = host.graph("peterson")
    m, mask, batch, obs = peterson_inputs()
    hidden_seen = 0
    for k, (lg, rows, o) in enumerate(zip(peterson_logs(), batch, obs)):
        for h in (lg[2], max(lg[2] - 1, 0)):
            v, path = behgap.hidden_path(m, rows, mask, hidden=h)
            assert v == bh.check(g, o, OBSERVED, False, h)[0]
            texts = [(slot, m.fmt(r), at) for slot, r, at in path]
            assert bh.path_ok(g, texts, o, OBSERVED, h), (k, h, texts)
            # one state per observation up to the deciding one, each gap with at most h hidden states
            assert sorted({at for _, _, at in path}) == list(range(v["step"])) and len(path) <= (h + 1) * max(v["step"], 1)
            assert behgap.hidden_path(m, rows, mask, hidden=h)[1] == path   # (the same on a second call)
            hidden_seen += len(path) - v["step"]
    assert hidden_seen > 50
    # without hidden steps it is the witness
    for rows in batch[:20]:
        _, _, wit = m.sets(rows, mask)
        assert [(s, r) for s, r, _ in behgap.hidden_path(m, rows, mask)[1]] == wit
        assert [at for _, _, at in behgap.hidden_path(m, rows, mask)[1]] == list(range(len(wit)))


def test_the_path_keeps_the_least_link_and_ends_in_the_least_row():
    gm = behgap.GapModel()
    # h = 1 is reached from h = 0 by work (slot 1) and by spin (slot 3), and from h = 2 by fold: least depth, then least slot
    v, path = gm.path((1, 0, 2, 0, behgap.ON_SPIN | behgap.ON_FOLD), behgap.xs(0, 1), behgap.X_ONLY, hidden=4)
    assert v["verdict"] == "accepted" and path == [(-1, (0, 0), 0), (1, (0, 1), 0), (1, (0, 2), 0), (0, (1, 0), 1)]
    # two members in the last set: the path ends in the lesser row
    v, path = gm.path((1, 0, 2, 0, 0), behgap.xs(0, 0), behgap.X_ONLY, hidden=1)
    assert v["candidates"] == 2 and path == [(-1, (0, 0), 0), (1, (0, 1), 1)]


def test_the_cases_of_the_test_lowering():
    gm = behgap.GapModel()
    for name, (case, batch, hidden, _, want) in behgap.GAP_CASES.items():
        assert gm.host(case, batch, behgap.X_ONLY, hidden=hidden) == want, name


# ------------------------------------------------------------------------------------------------ unlogged.tla and the command
def test_unlogged_tla_round_trip_and_verdicts():
    import tla_rust_amd as amd
    for cfg, accepted_at in (("unlogged", 2), ("unlogged_leaky", None)):
        prog = host.program("specs_behaviours/unlogged.tla", f"specs_behaviours/{cfg}.cfg")
        m = behshim.Model("pcal", prog.params)
        by_text, _ = m.reachable()
        assert len(by_text) == 5
        for row in by_text.values():   # format and parse are inverse on every reachable state
            text = amd.state_format("pcal", prog.params, row)
            assert amd.binding.state_parse("pcal", prog.params, text)[0] == row
        mask = prog.observe(["x"])
        log = [amd.binding.state_parse("pcal", prog.params, f"/\\ x = {x}")[0] for x in (0, 1, 3)]
        assert amd.binding.state_parse("pcal", prog.params, "/\\ x = 3")[1] == mask
        for h in (0, 1, 2, 3, 255):
            (v,) = behgap.hidden_check(m, [log], mask, hidden=h)
            assert v["verdict"] == ("accepted" if accepted_at is not None and h >= accepted_at else "rejected"), (cfg, h, v)
            assert v["verdict"] == "accepted" or v["step"] == 2


def test_cli_hidden_refusals(tmp_path):
    mc = ROOT / "tla_rust_amd" / "_build" / "mc"
    p = subprocess.run([str(mc), str(SB / "unlogged.tla"), "-hidden", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "-hidden needs -behaviours" in p.stderr, (p.stdout, p.stderr)
    for bad in ("256", "-1", "two"):
        p = subprocess.run([str(mc), str(SB / "unlogged.tla"), "-behaviours", "log.txt", "-hidden", bad], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "-hidden needs a number of unlogged steps between observations (0..255)" in p.stderr, (bad, p.stdout, p.stderr)


def test_the_binding_refuses_a_bound_past_255():
    import tla_rust_amd as amd
    with pytest.raises(ValueError, match="0 .. 255"):
        amd.binding.beh_flags(hidden=256)
    assert amd.binding.beh_flags(True, 255) == 1 | 255 << 8


# ------------------------------------------------------------------------------------------------ mutants
# name: (text of behaviour.h, its replacement, the case of behgap.GAP_CASES that must catch it)
MUTANTS = {
    "no-closure-dedup": ("if (m.fp == fp && beh_same_row(CWordRef{row, 1}, CWordRef{m.row.data(), 1}, W)) {", "if (false) {", "a hidden two-cycle"),
    "depth-off-by-one": ("const bool to_closure = depth < H && ", "const bool to_closure = depth <= H && ", "exactly G hidden steps, H = G - 1"),
    "intermediate-match-skipped": ("const bool to_closure = depth < H && beh_match(CWordRef{stage.data(), 1}, prev, mask, W);",
                                   "const bool to_closure = depth < H;", "an internal step that touches the logged word"),
    "closure-overflow-unnoticed": ("if (cur.size() + 1 > MC_BEH_MAX_CANDIDATES) return false;", "if (cur.size() + 1 > MC_BEH_MAX_CANDIDATES) return true;",
                                   "a closure of 65"),
    "closure-ambiguous-at-64": ("if (cur.size() + 1 > MC_BEH_MAX_CANDIDATES) return false;", "if (cur.size() + 1 >= MC_BEH_MAX_CANDIDATES) return false;",
                                "a closure of exactly 64"),
    "peak-without-the-closure": ("if (!ambiguous && cur.size() > v.peak) v.peak = (uint32_t)cur.size();", ";", "neighbouring lanes bring one closure row"),
    "joins-the-closure-only": ("if (to_next) {", "if (to_next && !to_closure) {", "a row that joins C and K at once"),
}


def test_mutants_are_caught(tmp_path):
    helpers.build_shim()

    def build(name):
        return behgap.build_host(csrc=testlib.mutant_tree(tmp_path, name, ("behaviour.h", *MUTANTS[name][:2])), out=tmp_path / name / "_build")
    good = behgap.GapModel()
    for name, so in testlib.build_mutants(MUTANTS, build).items():
        bad = behgap.GapModel()
        bad.L = behgap.load_host(so)
        case, batch, hidden, _, want = behgap.GAP_CASES[MUTANTS[name][2]]
        assert good.host(case, batch, behgap.X_ONLY, hidden=hidden) == want
        assert bad.host(case, batch, behgap.X_ONLY, hidden=hidden) != want, f"mutant {name} survives its case"
