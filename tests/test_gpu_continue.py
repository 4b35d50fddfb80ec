"""-continue on the device (MC_F_CONTINUE: k_viol_stored / k_viol_frontier of engine_violations.h, mc_engine_violations,
mc_engine_violation_trace, `mc X.tla -continue`) against the references of tests/contshim.py — the oracle's complete state graph for
the hand lowerings, oracle/tla_eval.py's Checker for compiled PlusCal: the summary entry by entry, a behaviour per entry that is a path
of the reference graph and ends in a violator, the counters of the whole search, the same first error as without the flag, every
route of the level loop, the budget stop, generated code, a clean model, together with -coverage, and mc's report."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

import contshim
import helpers
from test_continue_host import HAND, PCAL

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
pytestmark = pytest.mark.gpu
KW = dict(table_capacity=1 << 20, arena_capacity=1 << 18)
MC_F_NOBATCH = 256
CHECK_ON_EXPAND = {"ssi", "paxos"}


@pytest.fixture(scope="module")
def amd():
    import tla_rust_amd
    assert tla_rust_amd.device_count() >= 1, "no HIP device visible"
    return tla_rust_amd


_refs, _progs = {}, {}


def reference(name, tmp_path_factory):
    """the model's Reference, computed once for the module"""
    if name not in _refs:
        if name in HAND:
            spec, params, oparams, names, deadlock = HAND[name]
            _refs[name] = contshim.oracle_reference(spec, oparams, names, tmp_path_factory.mktemp(name), deadlock=deadlock,
                                                    check_on_expand=spec in CHECK_ON_EXPAND)
        else:
            text, invs, consts, cons, deadlock = contshim.module(name)
            host = helpers.ShimProgram(text, invariants=invs, constants=consts, constraints=cons)
            try:
                _refs[name] = contshim.checker_reference(host.translated(), consts, invs, constraints=cons, deadlock=deadlock)
            finally:
                host.close()
    return _refs[name]


def engine(amd, name, **kw):
    """an engine of the model (keyword arguments over KW); compiled programs stay alive with the module"""
    if name in HAND:
        spec, params, _o, _n, deadlock = HAND[name]
        return amd.Engine(spec, params, deadlock=deadlock, **{**KW, **kw})
    if name not in _progs:
        _progs[name] = amd.Program((contshim.SPECS / f"{name}.tla").read_text(), (contshim.SPECS / f"{name}.cfg").read_text())
    return amd.Engine("pcal", _progs[name].params, deadlock=contshim.module(name)[4], **{**KW, **kw})


def line(text):
    return text.replace("\n", " ")


def check_summary(name, v, ref):
    want = ref.entries()
    print(name, "engine", [dict(e) for e in v], "reference", want, "flagged levels", v.flagged_levels, "passes", v.passes)
    assert len(v) == len(want), (name, [e.kind for e in v], [e["kind"] for e in want])
    for got, w in zip(v, want):
        for key in ("kind", "name", "states", "outside", "first_level"):
            assert got[key] == w[key], f"{name}: {w['name']}.{key} = {got[key]}, the reference has {w[key]}"


def check_traces(name, eng, v, ref):
    for k, e in enumerate(v):
        if e.first_state is None:
            with pytest.raises(Exception):
                eng.violation_trace(k)
            continue
        tr = [line(t) for _a, t in eng.violation_trace(k)]
        rebuilt = e.kind == "invariant" and not e.fatal and e.states == 0
        assert len(tr) == e.trace_len == e.first_level + (1 if rebuilt else 0), (name, e.name, len(tr), e.trace_len, e.first_level)
        assert tr[0] in ref.init_texts, (name, e.name)
        for a, b in zip(tr, tr[1:]):
            assert b in ref.succ[a], (name, e.name, a, b)
        last = tr[-1]
        if e.fatal:    # the state whose expansion failed
            p = ref.index[last]
            assert any(par == p and f & 3 for par, f, _m, _i, _t in ref.edges), (name, last)
        elif e.kind == "deadlock":
            assert ref.dead[ref.index[last]], (name, last)
        elif rebuilt:   # a successor outside the model that breaks the invariant
            assert last not in ref.index and any(t == last and not m and i == e.invariant for _p, _f, m, i, t in ref.edges), (name, last)
        else:
            assert ref.breaks(last, e.invariant), (name, e.name, last)
        assert tr[len(tr) - 1 - (1 if rebuilt else 0)] == line(eng.state_texts(e.first_state, 1)[0])


def check_counters(name, r, ref):
    assert (r.distinct, r.generated, r.depth, r.levels) == (ref.distinct, ref.generated, ref.depth, ref.levels), \
        (name, r.distinct, r.generated, r.depth, ref.distinct, ref.generated, ref.depth)


@pytest.mark.parametrize("name", list(HAND) + PCAL)
def test_every_violation_of_the_search(amd, tmp_path_factory, name):
    """1 + 2: the summary, a behaviour per entry, the whole search's counters — and the first error is the one the same engine reports
    without the flag"""
    ref = reference(name, tmp_path_factory)
    eng = engine(amd, name, keep_going=True)
    try:
        r = eng.run()
        v = eng.violations()
        check_summary(name, v, ref)
        check_counters(name, r, ref)
        check_traces(name, eng, v, ref)
        assert v.flagged_levels > 0 and v.passes >= v.flagged_levels
        # (the behaviour's length is mc_engine_trace's: mc_result.trace_len of a violated initial state is 0 with and without the flag)
        first, first_raw = (r.verdict, r.violated_invariant, len(eng.trace())), (r.verdict, r.violated_invariant, r.trace_len)
    finally:
        eng.close()
    plain = engine(amd, name)
    try:
        p = plain.run()
        without, without_raw = (p.verdict, p.violated_invariant, len(plain.trace())), (p.verdict, p.violated_invariant, p.trace_len)
        with pytest.raises(Exception):
            plain.violations()   # MC_ESTATE: created without the flag
    finally:
        plain.close()
    errors = ref.first_errors()
    print(name, "first error with the flag", first, "without", without, "the first flagged level holds", errors)
    assert first in errors and without in errors
    if len(errors) == 1:
        assert first == without and first_raw == without_raw
    assert p.distinct <= r.distinct


def test_many_wrongs_stops_early_without_the_flag(amd, tmp_path_factory):
    eng = engine(amd, "many_wrongs")
    try:
        p = eng.run()
    finally:
        eng.close()
    assert (p.verdict, p.depth, p.distinct) == ("invariant", 3, 10)
    assert reference("many_wrongs", tmp_path_factory).distinct == 158


@pytest.mark.parametrize("name", ["ssi2x2", "ssi2x1"])
@pytest.mark.parametrize("route", ["chunks", "nobatch"])
def test_the_routes_of_the_level_loop_count_alike(amd, tmp_path_factory, name, route):
    """3: several chunks per level (the non-batched loop) and one host round trip per level"""
    ref = reference(name, tmp_path_factory)
    eng = engine(amd, name, keep_going=True, **(dict(chunk_states=1024) if route == "chunks" else dict(debug_flags=MC_F_NOBATCH)))
    try:
        r = eng.run()
        check_summary(name, eng.violations(), ref)
        check_counters(name, r, ref)
    finally:
        eng.close()


def test_a_budget_stop_counts_the_unexpanded_frontier(amd, tmp_path_factory):
    """4: max_levels stops ssi [2,1,127,1] on level 5: levels 1 - 4 are expanded, level 5's violators are counted all the same (the
    check_frontier path)"""
    ref = reference("ssi2x1", tmp_path_factory)
    eng = engine(amd, "ssi2x1", keep_going=True, max_levels=5)
    try:
        r = eng.run()
        v = eng.violations()
    finally:
        eng.close()
    want = [k for k in range(len(ref.level)) if ref.level[k] <= 5 and ref.inv[k] == 7]
    in_frontier = [k for k in want if ref.level[k] == 5]
    print("budget stop: counted", v[7].states, "of which the reference has", len(in_frontier), "in the unexpanded level 5")
    assert in_frontier and len(want) > len(in_frontier)
    assert (v[7].states, v[7].first_level) == (len(want), min(ref.level[k] for k in want))
    assert r.depth == 5 and r.distinct == sum(1 for lv in ref.level if lv <= 5) and r.queue_left == ref.levels[4]
    assert r.verdict == "invariant"


def test_generated_code_counts_alike(amd, tmp_path_factory):
    """5: many_wrongs as generated code (the SpecGenT instantiation of both kernels).  This test pays one hipcc build of the program's
    generated code (cached by the hash of its text)."""
    ref = reference("many_wrongs", tmp_path_factory)
    eng = engine(amd, "many_wrongs", keep_going=True, jit=True)
    try:
        r = eng.run()
        v = eng.violations()
        check_summary("many_wrongs/jit", v, ref)
        check_counters("many_wrongs/jit", r, ref)
        check_traces("many_wrongs/jit", eng, v, ref)
    finally:
        eng.close()


def test_a_clean_model_launches_nothing(amd):
    """6: atomic_add [3] has no violation: no flagged level, no launch, every row zero"""
    eng = amd.Engine("atomic_add", [3], keep_going=True, **KW)
    plain = amd.Engine("atomic_add", [3], **KW)
    try:
        r, p = eng.run(), plain.run()
        v = eng.violations()
    finally:
        eng.close()
        plain.close()
    assert (v.passes, v.flagged_levels) == (0, 0)
    assert [e.kind for e in v] == ["deadlock"] and all(e.states == 0 and e.outside == 0 and e.first_state is None for e in v)
    assert r.verdict == "ok" and (r.distinct, r.generated, r.depth, r.levels) == (p.distinct, p.generated, p.depth, p.levels)


def test_with_coverage_the_sums_are_the_results(amd, tmp_path_factory):
    """7: MC_F_CONTINUE | MC_F_COVERAGE: the coverage counts go on with the search"""
    ref = reference("many_wrongs", tmp_path_factory)
    eng = engine(amd, "many_wrongs", keep_going=True, coverage=True)
    try:
        r = eng.run()
        cov = eng.coverage()
        check_summary("many_wrongs/coverage", eng.violations(), ref)
    finally:
        eng.close()
    assert sum(d for d, _g in cov.values()) == r.distinct == ref.distinct
    assert sum(g for _d, g in cov.values()) == r.generated == ref.generated


def test_mc_continue_report(amd, tmp_path_factory):
    """8: `mc many_wrongs.tla -continue`: exit 12, the first error as ever, the block's lines, each listed behaviour's length, and
    the closing count line of the whole search"""
    ref = reference("many_wrongs", tmp_path_factory)
    p = subprocess.run([str(ROOT / "tla_rust_amd" / "_build" / "mc"), str(contshim.SPECS / "many_wrongs.tla"), "-continue", "-noprogress"],
                       capture_output=True, text=True, timeout=600)
    print(p.stdout[-6000:], p.stderr[-2000:])
    assert p.returncode == 12, (p.returncode, p.stderr)
    out = p.stdout
    assert out.index("Error: Invariant LockFree is violated.") < out.index("a state is listed under its first violated invariant only")
    block = out[out.index("a state is listed under its first violated invariant only"):]
    by = {e["name"]: e for e in ref.entries()}
    for nm in ("LockFree", "Small", "Fresh"):
        assert f"Invariant {nm}: {by[nm]['states']} distinct states, first at depth {by[nm]['first_level']}\n" in block, nm
    assert "Invariant Both: 0 distinct states\n" in block
    assert f"Deadlock: {by['Deadlock']['states']} distinct states, first at depth {by['Deadlock']['first_level']}\n" in block
    # under each line that is not the first error: its behaviour, first_level states long
    parts = re.split(r"^(Invariant \w+|Deadlock): .*$", block, flags=re.M)
    shown = {parts[k].split()[-1]: len(re.findall(r"^State \d+: <", parts[k + 1], flags=re.M)) for k in range(1, len(parts) - 1, 2)}
    assert shown == {"LockFree": 0, "Small": by["Small"]["first_level"], "Fresh": by["Fresh"]["first_level"], "Both": 0,
                     "Deadlock": by["Deadlock"]["first_level"]}, shown
    assert f"{ref.generated} states generated, 158 distinct states found, 0 states left on queue.\n" in block
    first = out[:out.index("The search continued")]
    assert len(re.findall(r"^State \d+: <", first, flags=re.M)) == 3


def test_a_sharded_engine_refuses_the_flag(amd):
    with pytest.raises(Exception) as e:
        amd.Engine("atomic_add", [3], keep_going=True, shard_rank=0, shard_count=2, **KW)
    assert "MC_F_CONTINUE: not available for a sharded engine" in str(e.value)
