"""The state graph on the device (k_graph_index / k_graph_degree / k_graph_fill of engine_graph.h, mc_engine_graph, `mc X.tla -dump dot`)
against the oracle's state graph, BY STATE TEXT: the multiset {(source text, action name, destination text)} of Engine.graph() equals the
oracle's edges without an Assert / evaluation-error flag whose successor is in-model and stored within the levels kept — at every budget,
on a violating model, next to -coverage's counts, over a seen-set near its load limit, across mc_engine_step, on compiled programs
(interpreter = generated code = oracle/tla_eval.py), and in mc's dot file.  The order of a level's states in the arena is the engine's
race: nothing here compares indices between two runs."""
import re
import subprocess
import sys
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import graphshim
import helpers
from test_gpu_coverage import CLEAN, KW, RAFT, graph, model, program

ROOT = Path(__file__).resolve().parent.parent
S = ROOT / "specs"
sys.path.insert(0, str(ROOT / "oracle"))
pytestmark = pytest.mark.gpu
MC_EBADCFG, MC_ESTATE = -1, -7


@pytest.fixture(scope="module")
def amd():
    import tla_rust_amd
    assert tla_rust_amd.device_count() >= 1, "no HIP device visible"
    return tla_rust_amd


def check_arrays(info, offsets, dst, act, r):
    """what holds for every graph, from the arrays alone"""
    assert info.states == r.distinct and len(offsets) == info.states + 1 and len(dst) == len(act) == info.edges
    off = offsets.astype(np.int64)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == info.edges
    deg = np.diff(off)
    assert info.max_out_degree == (deg.max() if len(deg) else 0)
    src = np.repeat(np.arange(info.states, dtype=np.int64), deg)
    assert info.self_loops == int((src == dst.astype(np.int64)).sum())
    assert (dst.astype(np.int64) < info.states).all() and info.expanded <= info.states
    assert (deg[info.expanded:] == 0).all(), "a state of the unexpanded last level has out-edges"
    return deg


def check_against_oracle(g, eng, r, expanded):
    """eng: an engine whose search expanded levels 1 .. expanded (None: all) and returned r; returns (info, multiset, texts, degrees)"""
    info, offsets, dst, act = eng.graph()
    deg = check_arrays(info, offsets, dst, act, r)
    got, texts = graphshim.engine_edges(eng, info, offsets, dst, act)
    want = graphshim.oracle_edges(g, expanded)
    levels = [lv for lv in g.level if expanded is None or lv <= expanded + 1]
    print("levels", expanded, dict(info), "oracle edges", sum(want.values()))
    assert info.states == len(levels) and info.init_states == sum(1 for lv in levels if lv == 1)
    assert info.expanded == sum(1 for lv in levels if expanded is None or lv <= expanded)
    assert sorted(texts) == sorted(t for t, lv in zip(g.text, g.level) if expanded is None or lv <= expanded + 1)
    assert got == want, (f"{sum(got.values())} edges, the oracle's graph has {sum(want.values())}; only here: {list((got - want).items())[:3]}; "
                         f"only there: {list((want - got).items())[:3]}")
    init_generated = sum(1 for e in g.edges if e[0] < 0)
    assert init_generated + info.edges + info.dropped == r.generated
    return info, got, texts, deg


@pytest.mark.parametrize("key", CLEAN)
def test_edges_are_the_oracles_at_every_budget(amd, tmp_path_factory, key):
    spec, params, oparams, deadlock = model(amd, key)
    g = graph(tmp_path_factory, spec, oparams, deadlock)
    for ml in sorted({0, 3, g.depth - 1}):   # unlimited; two budgets: early, and all but the last level (one budget where they coincide)
        eng = amd.Engine(spec, params, deadlock=deadlock, max_levels=ml, **KW)
        r = eng.run()
        try:
            if ml:
                assert r.verdict == "budget" and len(r.levels) == ml
            # max_levels = M: levels 1 .. M - 1 were expanded, level M was found and is the queue
            info, _, _, _ = check_against_oracle(g, eng, r, ml - 1 if ml else None)
            assert (info.expanded == info.states) == (not ml) and info.states - info.expanded == r.queue_left
        finally:
            eng.close()


def test_the_graph_stops_at_the_end_of_the_violating_level(amd, tmp_path_factory):
    spec, params, oparams, deadlock = model(amd, "pcal_intro_readme")   # the Assert at C fails
    g = graph(tmp_path_factory, spec, oparams, deadlock)
    o = helpers.oracle_run(spec, oparams, stop=1)   # stops at the end of the level that found the violation
    assert o["verdict"] == "assert"
    expanded = [e for e in range(1, g.depth + 1) if sum(g.generated(e).values()) == o["generated"]]
    assert len(expanded) >= 1
    eng = amd.Engine(spec, params, **KW)
    r = eng.run()
    try:
        assert (r.verdict, r.generated, r.distinct) == (o["verdict"], o["generated"], o["distinct"])
        info, _, _, _ = check_against_oracle(g, eng, r, expanded[0])
        assert info.dropped > 0   # the failed Asserts: generated, no successor state
        flagged = sum(1 for par, _, flags, _, _ in g.edges if par >= 0 and flags & 3 and g.level[par] <= expanded[0])
        assert info.dropped >= flagged > 0
    finally:
        eng.close()


@pytest.mark.parametrize("key", ["raft2", "pcal_intro_readme"])
def test_per_action_edges_and_coverage(amd, key):
    """for every action: its edges <= the successors it generated, and the deficits sum to `dropped`"""
    spec, params, _, deadlock = model(amd, key)
    eng = amd.Engine(spec, params, deadlock=deadlock, coverage=True, **KW)
    r = eng.run()
    try:
        cov = eng.coverage()
        info, offsets, dst, act = eng.graph()
        check_arrays(info, offsets, dst, act, r)
        import ctypes as C
        import tla_rust_amd.binding as b
        per = Counter(b.lib().mc_action_name(C.byref(eng.desc), a).decode() for a in act.tolist())
        assert set(per) <= set(cov) - {"Init"}
        deficit = 0
        for name, (_, generated) in cov.items():
            if name != "Init":
                assert per[name] <= generated, (name, per[name], generated)
                deficit += generated - per[name]
        assert deficit == info.dropped and cov["Init"][1] + info.edges + info.dropped == r.generated
    finally:
        eng.close()


def test_a_table_near_its_load_limit(amd, tmp_path_factory):
    """the dense bucket form (KW's table is >= 3 x its arena: every other test here probes 4-slot buckets) at the load
    mc_engine_restore still accepts, 0.9 (engine.hip: `h.distinct * 10 > table_cap * 9`): most keys have left their home bucket"""
    spec, params, oparams, deadlock = model(amd, "raft2")
    g = graph(tmp_path_factory, spec, oparams, deadlock)
    n = len(g.text)
    eng = r = None
    for load in (0.9, 0.8):   # (the next size up if the search itself finds the table full; no third try)
        cap = (int(n / load) + 63) // 64 * 64
        assert cap < 3 * KW["arena_capacity"]   # the dense form
        eng = amd.Engine(spec, params, deadlock=deadlock, **dict(KW, table_capacity=cap))
        try:
            r = eng.run()
            break
        except amd.McError as e:
            eng.close()
            eng = None
            assert e.code == -4, e   # MC_ETABLEFULL
    assert eng is not None, "the table was full at load 0.8 too"
    try:
        check_against_oracle(g, eng, r, None)
    finally:
        eng.close()


@pytest.mark.parametrize("key,some", [("atomic_add3", False), ("voting", True)])
def test_terminal_states_have_empty_rows(amd, tmp_path_factory, key, some):
    """with deadlock checking off a search passes through its terminal states: their rows, inside an expanded level, are empty, and no
    other row is.  atomic_add [3] has no terminal state — the oracle's graph has an edge out of every one of its 9 states, the last one
    stutters (Terminating) — so for it the equivalence holds with both sides empty; the Voting model has 22 terminal states of 599."""
    spec, params, oparams, _ = model(amd, key)
    g = graph(tmp_path_factory, spec, oparams, False)
    eng = amd.Engine(spec, params, deadlock=False, **KW)
    r = eng.run()
    try:
        assert r.verdict == "ok"
        info, got, texts, deg = check_against_oracle(g, eng, r, None)
        assert info.expanded == info.states
        with_edges = {a for (a, _, _) in graphshim.oracle_edges(g)}
        terminal = [t for t in g.text if t not in with_edges]
        print(key, len(terminal), "terminal states of", len(g.text))
        assert sorted(t for t, d in zip(texts, deg) if d == 0) == sorted(terminal) and (len(terminal) > 0) == some
    finally:
        eng.close()


def test_graph_between_two_steps(amd):
    spec, params = "raft", RAFT
    whole = amd.Engine(spec, params, **KW)
    rw = whole.run()
    iw, ow, dw, aw = whole.graph()
    gw, _ = graphshim.engine_edges(whole, iw, ow, dw, aw)
    whole.close()
    eng = amd.Engine(spec, params, **KW)
    try:
        r1 = eng.step(5)
        i1, o1, d1, a1 = eng.graph()
        g1, t1 = graphshim.engine_edges(eng, i1, o1, d1, a1)
        assert r1.verdict == "budget" and i1.states == r1.distinct and 0 < i1.expanded < i1.states
        again = eng.graph()   # a second build of the same search: the same arrays, index by index
        assert (again[1] == o1).all() and (again[2] == d1).all() and (again[3] == a1).all()
        r2 = eng.step(4096 - 8)   # the continued search: what an uninterrupted run returns
        assert (r2.verdict, r2.distinct, r2.generated, r2.depth, r2.levels) == (rw.verdict, rw.distinct, rw.generated, rw.depth, rw.levels)
        with pytest.raises(amd.McError) as e:   # the step released the graph
            eng.graph_read(0, 1, 16)
        assert e.value.code == MC_ESTATE
        i2, o2, d2, a2 = eng.graph()
        g2, _ = graphshim.engine_edges(eng, i2, o2, d2, a2)
        assert g2 == gw and (i2.states, i2.edges, i2.self_loops, i2.dropped) == (iw.states, iw.edges, iw.self_loops, iw.dropped)
        first_sources = set(t1[:i1.expanded])   # where the two graphs overlap: the rows of the states the first search had expanded
        assert Counter({k: n for k, n in g2.items() if k[0] in first_sources}) == g1
    finally:
        eng.close()


def test_refusals_are_error_codes(amd):
    eng = amd.Engine("atomic_add", [3], **KW)
    try:
        with pytest.raises(amd.McError) as e:   # before the first run
            eng.graph_info()
        assert e.value.code == MC_ESTATE
        with pytest.raises(amd.McError) as e:
            eng.graph_read(0, 1, 16)
        assert e.value.code == MC_ESTATE
        r = eng.run()
        info = eng.graph_info()
        assert info.states == r.distinct == 9 and info.edges > 0
        with pytest.raises(amd.McError) as e:   # a short buffer: MC_EBADCFG, and the message has the count
            eng.graph_read(0, info.states, info.edges - 1)
        assert e.value.code == MC_EBADCFG and f"({info.edges} edges)" in str(e.value)
        with pytest.raises(amd.McError) as e:   # a range beyond the graph
            eng.graph_read(info.states, 1, 16)
        assert e.value.code == MC_EBADCFG
        off, dst, act = eng.graph_read(info.states, 0, 0)   # the empty range at the end is one
        assert list(off) == [0] and len(dst) == 0
        assert eng.run().distinct == 9   # refusals and reads left the engine as it was
        eng.simulate(64, depth=5, seed=1)
        with pytest.raises(amd.McError) as e:   # after a simulation
            eng.graph_info()
        assert e.value.code == MC_ESTATE
    finally:
        eng.close()
    sharded = amd.Engine("atomic_add", [3], shard_rank=0, shard_count=2, **KW)
    try:
        with pytest.raises(amd.McError) as e:
            sharded.graph_info()
        assert e.value.code == MC_EBADCFG and "sharded" in str(e.value)
    finally:
        sharded.close()


def test_a_restored_engine_has_no_graph_until_it_runs(amd, tmp_path):
    a = amd.Engine("raft", RAFT, max_levels=7, **KW)
    assert a.run().verdict == "budget"
    a.checkpoint(tmp_path / "raft.ck")
    a.close()
    b = amd.Engine("raft", RAFT, **KW)
    try:
        b.restore(tmp_path / "raft.ck")
        with pytest.raises(amd.McError) as e:
            b.graph_info()
        assert e.value.code == MC_ESTATE
        r = b.run()
        info = b.graph_info()
        assert info.states == r.distinct == info.expanded
    finally:
        b.close()


def checker_pairs(prog, consts, invs):
    """{(source text, destination text): n} of oracle/tla_eval.py's graph of the program's translation (simgraph.from_checker: its edges
    carry no action name): unflagged edges to in-model successors, which a complete search stores"""
    import simgraph
    from tla_eval import Checker
    g = simgraph.from_checker(Checker(prog.translated(), constants=consts), invariants=invs)
    return Counter((s, e.text) for s, es in g.succ.items() for e in es if not e.flags & 3 and e.inmodel and e.text in g.succ), g


def test_a_compiled_program_interpreted_and_as_generated_code(amd):
    """csyntax_mix: an either and a with, several slots per label"""
    from test_pcal import CASES
    prog, path, consts = program(amd, "csyntax_mix")
    invs = next(c[1] for c in CASES if c[0] == path)
    try:
        want, g = checker_pairs(prog, consts, invs)
        for jit in (False, True):
            eng = amd.Engine("pcal", prog.params, jit=jit, **KW)
            try:
                r = eng.run()
                info, offsets, dst, act = eng.graph()
                check_arrays(info, offsets, dst, act, r)
                got, texts = graphshim.engine_edges(eng, info, offsets, dst, act)
                assert r.verdict == "ok" and sorted(texts) == sorted(g.succ)
                pairs = Counter()
                for (a, _, b), n in got.items():
                    pairs[(a, b)] += n
                assert pairs == want, (jit, sum(pairs.values()), sum(want.values()))
                assert len(g.init) + info.edges + info.dropped == r.generated
                assert "Done" not in {name for _, name, _ in got}
            finally:
                eng.close()
    finally:
        prog.close()


def test_three_engines_of_three_units_share_the_graph_passes(amd):
    """The passes over the CSR arrays (reads, components, the fairness check) are compiled once for the library and serve the engine of
    every translation unit: a hand lowering's (atomic_add), another one's (the Voting model of 77 states under SYMMETRY) and the unit of
    generated code built at load time (two_loops, jit).  Three engines alive at once, their calls interleaved: each gets what it gets
    alone, so the shared object keeps nothing between calls.  (The sweep counts of mc_scc_info are left out: sweeps update in place, and
    how many it takes to reach the fixed point is the wavefronts' race; `seconds` is a time.)"""
    import livegraph
    m = livegraph.MODELS["two_loops"]
    prog = amd.Program((livegraph.DIR / m.tla).read_text(), (livegraph.DIR / m.cfg).read_text())
    engines = [amd.Engine("atomic_add", [3], **KW), amd.Engine("paxos", [1, 3, 2, 2, 1, 3, 1], deadlock=False, **KW),
               amd.Engine("pcal", prog.params, jit=True, **KW)]
    a, v, t = engines
    ginfo = lambda i: {k: x for k, x in dict(i).items() if k != "seconds"}   # noqa: E731
    sinfo = lambda i: {k: x for k, x in dict(i).items() if k != "seconds" and not k.endswith("_rounds")}   # noqa: E731
    try:
        results = [e.run() for e in engines]
        assert [r.verdict for r in results] == ["ok"] * 3 and [r.distinct for r in results[:2]] == [9, 77]
        alone = []
        for e in engines:   # one engine at a time: graph, components
            info, offsets, dst, act = e.graph()
            si, scc = e.scc()
            alone.append((ginfo(info), offsets, dst, act, sinfo(si), scc))
        assert alone[2][4]["nontrivial"] == 3
        li = t.liveness(prog.fair_mask)
        trace = t.liveness_trace()
        assert li.violated == 1 and trace[0]
        # interleaved: every build of one engine between two of another
        gi = {}
        for e in (t, a, v):
            gi[e] = ginfo(e.graph_info())
        si = {}
        for e in (v, t, a):
            si[e] = e.scc()
        for e in (a, v, t):
            info, offsets, dst, act = e.graph()                  # (rebuilds: the components above are released with the old graph)
            g0, o0, d0, a0, s0, c0 = alone[engines.index(e)]
            assert gi[e] == g0 == ginfo(info) and (offsets == o0).all() and (dst == d0).all() and (act == a0).all()
            assert sinfo(si[e][0]) == s0 and (si[e][1] == c0).all()
        # the fairness check of one engine around the others' calls
        assert dict(t.liveness(prog.fair_mask), seconds=0) == dict(li, seconds=0)
        a.scc()
        v.graph_info()
        assert t.liveness_trace() == trace
        v.scc()
        assert dict(t.liveness(prog.fair_mask), seconds=0) == dict(li, seconds=0) and t.liveness_trace() == trace
        assert (a.scc()[1] == alone[0][5]).all() and (v.scc()[1] == alone[1][5]).all() and (t.scc()[1] == alone[2][5]).all()
        print("two_loops", dict(t.graph_info()), dict(t.scc()[0]))
    finally:
        for e in engines:
            e.close()
        prog.close()


# ------------------------------------------------------------------------------------------------ mc
NODE = re.compile(r'^(\d+) \[label="((?:[^"\\]|\\.)*)"(,style = filled)?\]$')
EDGE = re.compile(r'^(\d+) -> (\d+)(?: \[label="((?:[^"\\]|\\.)*)"\])?;$')


def unescape(s):
    return re.sub(r"\\(.)", lambda m: "\n" if m.group(1) == "n" else m.group(1), s)


def read_dot(path):
    lines = path.read_text().splitlines()
    assert lines[:4] == ["strict digraph DiskGraph {", "nodesep=0.35;", "subgraph cluster_graph {", 'color="white";'] and lines[-2:] == ["}", "}"]
    nodes, filled, edges = {}, set(), []
    for ln in lines[4:-2]:
        m = NODE.match(ln)
        if m:
            assert int(m.group(1)) not in nodes
            nodes[int(m.group(1))] = unescape(m.group(2))
            if m.group(3):
                filled.add(int(m.group(1)))
            continue
        m = EDGE.match(ln)
        assert m, ln
        edges.append((int(m.group(1)), int(m.group(2)), None if m.group(3) is None else unescape(m.group(3))))
    return nodes, filled, edges


def read_dump(path):
    text = path.read_text()
    parts = re.split(r"^State (\d+):\n", text, flags=re.M)
    assert parts[0] == "" and all(p.endswith("\n\n") for p in parts[2::2])   # "State k:\n" + the variables + a blank line
    return {int(k): body[:-2] for k, body in zip(parts[1::2], parts[2::2])}


def run_mc(*args):
    mc = ROOT / "tla_rust_amd" / "_build" / "mc"
    assert mc.exists(), "build() has not run"
    return subprocess.run([str(mc), *map(str, args), "-noprogress"], capture_output=True, text=True, timeout=600)


def test_mc_dump_dot(amd, tmp_path):
    from test_pcal import CASES
    tla = S / "pluscal" / "peterson.tla"
    p = run_mc(tla, "-dump", "dot,actionlabels", tmp_path / "g.dot", "-dump", tmp_path / "states.txt")
    assert p.returncode == 0, (p.stdout, p.stderr)
    nodes, filled, edges = read_dot(tmp_path / "g.dot")
    states = read_dump(tmp_path / "states.txt")
    assert nodes == states and sorted(nodes) == list(range(1, len(nodes) + 1))   # node k IS "State k:" of the plain dump
    # the oracle: tla_eval's graph of the translation; a strict digraph has one edge per (source, destination)
    prog, path, consts = program(amd, "peterson")
    invs = next(c[1] for c in CASES if c[0] == path)
    try:
        want, g = checker_pairs(prog, consts, invs)
        one_line = {k: t.replace("\n", " ") for k, t in nodes.items()}
        assert sorted(one_line.values()) == sorted(g.succ)
        assert {(one_line[a], one_line[b]) for a, b, _ in edges} == set(want)
        assert {one_line[k] for k in filled} == {e.text for e in g.init}
        eng = amd.Engine("pcal", prog.params, **KW)
        r = eng.run()
        info = eng.graph_info()
        eng.close()
    finally:
        prog.close()
    assert all(lab for _, _, lab in edges) and len(edges) == info.edges
    lines = p.stdout.splitlines()
    k = lines.index(f"The depth of the complete state graph search is {r.depth}.")
    assert lines[k + 1] == f"The state graph has {info.states} states and {info.edges} transitions ({info.self_loops} self loops)."
    # plain -dump: the file's layout is what it was, and the report has no graph line
    q = run_mc(tla, "-dump", tmp_path / "plain.txt")
    assert q.returncode == 0 and "The state graph has" not in q.stdout and q.stdout.splitlines() == lines[:k + 1] + lines[k + 2:]
    plain = read_dump(tmp_path / "plain.txt")
    assert sorted(plain) == sorted(states) and sorted(plain.values()) == sorted(states.values())
    assert (tmp_path / "plain.txt").read_text() == "".join(f"State {k}:\n{plain[k]}\n\n" for k in sorted(plain))
    # colorize: colours on the edges and a legend of the actions used
    c = run_mc(tla, "-dump", "dot,actionlabels,colorize", tmp_path / "c.dot")
    assert c.returncode == 0
    text = (tmp_path / "c.dot").read_text()
    assert 'color="' in text and 'fontcolor="' in text and "subgraph cluster_legend {" in text and text.endswith("}\n}\n")
    for lab in {lab for _, _, lab in edges}:
        assert f'"{lab}" [label="{lab}",fillcolor=' in text


def test_mc_dump_dot_of_a_recovered_search(tmp_path):
    """-checkpoint and -recover pass through: the graph of a recovered search that ran on has the checkpointed levels' edges too"""
    tla = S / "pluscal" / "peterson.tla"
    whole = run_mc(tla, "-dump", "dot,actionlabels", tmp_path / "whole.dot")
    assert whole.returncode == 0, (whole.stdout, whole.stderr)
    a = run_mc(tla, "-maxlevels", 4, "-checkpoint", tmp_path / "p.ck", "-dump", "dot", tmp_path / "part.dot")
    assert a.returncode == 0 and "-- Checkpointing of run" in a.stdout, (a.stdout, a.stderr)
    part_nodes, _, part_edges = read_dot(tmp_path / "part.dot")
    b = run_mc(tla, "-recover", tmp_path / "p.ck", "-dump", "dot,actionlabels", tmp_path / "rec.dot")
    assert b.returncode == 0, (b.stdout, b.stderr)
    (wn, wf, we), (rn, rf, re_) = read_dot(tmp_path / "whole.dot"), read_dot(tmp_path / "rec.dot")
    by_text = lambda nodes, edges: Counter((nodes[x], lab, nodes[y]) for x, y, lab in edges)
    assert sorted(wn.values()) == sorted(rn.values()) and by_text(wn, we) == by_text(rn, re_) and {wn[k] for k in wf} == {rn[k] for k in rf}
    assert 0 < len(part_nodes) < len(wn) and 0 < len(part_edges) < len(we)
    graph_line = [ln for ln in b.stdout.splitlines() if ln.startswith("The state graph has")]
    assert graph_line == [ln for ln in whole.stdout.splitlines() if ln.startswith("The state graph has")] and len(graph_line) == 1
