"""What the state graph is made of, on the host (tla_rust_amd/csrc/graph.h through tests/_graphshim, no GPU), against the ORACLE'S STATE
GRAPH: the seen-set lookup and the edge rule the device kernels run (engine_graph.h) are run here over every state of a host search
whose fingerprints lie in a table of the seen-set's exact layout — both bucket widths, and small enough that keys leave their home
bucket — and the edge multiset {(source text, action name, destination text)} must be the oracle's: its edges without an Assert /
evaluation-error flag whose successor is in-model and stored.  States are compared by text, never by index.

Mutants of graph.h (test_mutants_are_killed builds each and asserts that the check fails) and what kills each:
  find-stops-at-home    seen_find gives up after the home bucket       every model: a key that overflowed its bucket is "missing"
  selfloop-dropped      the edge rule drops self loops                 raft / pcal_intro: the stuttering edges are short
  flagged-looked-up     a failed Assert's key is looked up             the README's pcal_intro: 220 edges to states the failed steps never reached, 110 keys "missing"
"""
import pytest

import covshim
import graphshim
import helpers
import testlib

ROOT = helpers.ROOT
RAFT = [2, 2, 2, 9, 1, 1]
MODELS = [
    ("atomic_add", [3], [3], True),
    ("pcal_intro", [0, 1, 20, 2], [0, 1, 20, 2], True),
    ("raft", RAFT, helpers.raft_oracle_params(RAFT), True),      # 2 servers: self loops, out-of-model successors
    ("ssi", [2, 2, 127, 0], [2, 2, 127, 0], True),
    ("pcal_intro", [1, 0, 20, 2], [1, 0, 20, 2], True),          # the README's Assert fails: flagged successors are dropped
]
IDS = [f"{s}{p}" for s, p, _, _ in MODELS]
_graphs = {}


def oracle(tmp_path_factory, spec, oparams, deadlock):
    k = (spec, tuple(oparams), deadlock)
    if k not in _graphs:   # computed once, shared, never changed
        _graphs[k] = covshim.OracleGraph(spec, oparams, tmp_path_factory.mktemp("oracle"), check_deadlock=deadlock)
    return _graphs[k]


def tight_buckets(states, slots):
    """a table at load 0.85: with 8 (4) slots per bucket about a bucket in four (three) is full, and its later keys move on"""
    return max(2, int(states / (0.85 * slots)) + 1)


def check_model(g, tmp, spec, params, sparse, L=None):
    slots = 4 if sparse else 8
    nb = tight_buckets(len(g.text), slots)
    counts, texts, got = graphshim.search(spec, params, nb, sparse, tmp, L=L)
    want = graphshim.oracle_edges(g)
    print(spec, params, "sparse" if sparse else "dense", nb, "buckets", counts, "oracle edges", sum(want.values()))
    assert counts["missing"] == 0, f"{counts['missing']} keys the search stored are not found again"
    assert sorted(texts) == sorted(g.text)
    assert got == want, (f"{sum(got.values())} edges, the oracle's graph has {sum(want.values())}; "
                         f"only here: {list((got - want).items())[:3]}; only there: {list((want - got).items())[:3]}")
    assert counts["edges"] == sum(want.values())
    assert counts["self_loops"] == sum(n for (a, _, b), n in want.items() if a == b)
    # every generated successor is an initial state, an edge, or dropped: the invariant mc_engine_graph documents
    init = sum(1 for e in g.edges if e[0] < 0)
    assert counts["generated"] == g.counters["generated"] == len(g.edges)
    assert init + counts["edges"] + counts["dropped"] == counts["generated"]
    if len(g.text) > 100:
        assert counts["left_home"] > 0, "the table is too roomy for this test: no key left its home bucket"
    return counts


@pytest.mark.parametrize("sparse", [False, True], ids=["8slots", "4slots"])
@pytest.mark.parametrize("spec,params,oparams,deadlock", MODELS, ids=IDS)
def test_host_graph_is_the_oracles(tmp_path, tmp_path_factory, spec, params, oparams, deadlock, sparse):
    check_model(oracle(tmp_path_factory, spec, oparams, deadlock), tmp_path, spec, params, sparse)


def test_a_roomy_table_gives_the_same_graph(tmp_path, tmp_path_factory):
    spec, params, oparams, deadlock = MODELS[2]
    g = oracle(tmp_path_factory, spec, oparams, deadlock)
    counts, _, got = graphshim.search(spec, params, 1 << 16, True, tmp_path)
    assert counts["missing"] == 0 and got == graphshim.oracle_edges(g)


# ------------------------------------------------------------------------------------------------ mutants
# name: (its text in graph.h, the replacement, the model of MODELS that must fail, what the failure must say)
MUTANTS = {
    "find-stops-at-home": ("bk = bk + 1 == nbuckets ? 0 : bk + 1;", "return GRAPH_ABSENT;", 2, "are not found again"),
    "selfloop-dropped": ("if (st & ST_SELFLOOP) return GE_SELF;", "if (st & ST_SELFLOOP) return GE_DROPPED;", 2, "edges, the oracle's graph has"),
    "flagged-looked-up": ("if (st & (ST_ASSERT | ST_SPECERR | ST_OVERFLOW)) return GE_DROPPED;", "", 4, "are not found again"),
}


def test_mutants_are_killed(tmp_path, tmp_path_factory):
    helpers.build_shim()

    def build(name):
        return graphshim.build_graphshim(csrc=testlib.mutant_tree(tmp_path, name, ("graph.h", *MUTANTS[name][:2])), out=tmp_path / name / "_build")
    for name, so in testlib.build_mutants(MUTANTS, build).items():
        _, _, model, says = MUTANTS[name]
        spec, params, oparams, deadlock = MODELS[model]
        d = tmp_path / name / "run"
        d.mkdir()
        with pytest.raises(AssertionError) as e:
            check_model(oracle(tmp_path_factory, spec, oparams, deadlock), d, spec, params, False, L=graphshim.load(so))
            pytest.fail(f"mutant {name} survives", pytrace=False)
        assert says in str(e.value), (name, str(e.value)[:300])
    # ... and the product's own header passes where they fail
    for model in sorted({m[2] for m in MUTANTS.values()}):
        spec, params, oparams, deadlock = MODELS[model]
        d = tmp_path / f"product{model}"
        d.mkdir()
        check_model(oracle(tmp_path_factory, spec, oparams, deadlock), d, spec, params, False)
