"""Host-side pieces of bench.py that run without a GPU: the workload table against the golden files, the kernel-source stamp of the
counter summary the contract line quotes, the N-rank line's HBM figure."""
import importlib.util
import json
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", ROOT / "bench.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_every_workload_names_a_golden_case():
    b = _bench()
    for name, w in b.WORKLOADS.items():
        g = json.loads((ROOT / "tests" / "golden" / w.get("golden_file", "raft_levels.json")).read_text())
        case = next(c for c in g["cases"] if c["name"] == w["golden"])
        assert case["distinct"] > 0 and len(case["levels"]) == case["depth"], name
        if "max_levels" in w:
            assert case["depth"] == w["max_levels"] and case["verdict"] == w["verdict"] == "budget", name


def test_the_quoted_counter_summary_is_stamped_with_the_kernel_sources_of_this_tree():
    """bench.py reads HBM traffic from the newest profiles/r*_pmc.json of the workload's SPEC and refuses it (traffic = null) unless it was
    collected on the kernel sources that are timed: a commit that touches the kernels without re-collecting the counters shows up here
    (as a SKIP naming the stale summary), not only in the driver's line"""
    import pytest
    b = _bench()
    stale = []
    for spec, stag, kn in (("raft", "SpecRaft<3>", ("k_expand_family",)), ("raft", "SpecRaft<5>", ("k_expand_family",)), ("ssi", "SpecSsi", ("k_expand_pairs",))):
        src, k = b.pmc_for(spec, stag, kn)
        if k is None:   # (between a kernel change and its next profile this is a state of work, not an error: the line then says traffic = null)
            stale.append(f"{stag}: {src}")
        else:
            assert k["launches"] > 0 and "FETCH_SIZE" in k and "WRITE_SIZE" in k, (stag, src)
    if stale:
        pytest.skip("; ".join(stale) + ": re-run profiles/collect.sh")


def test_n_rank_roofline_object():
    b = _bench()
    import tla_rust_amd as amd
    W = amd.state_bytes("raft", b.WORKLOADS["t3"]["params"])
    r = b.dist_roofline(W, 525782408, 6708500293, 8, 0.025)
    assert W == 136 and r["bound"] == "hbm" and r["peak"] == 8000.0 and r["traffic"] is None
    assert abs(r["alg_bytes_per_step_per_gpu"] - (2 * 136 * 525782408 + 8 * 6708500293) / 8) < 1 and abs(r["frac"] - r["achieved"] / 8000.0) < 1e-12
    assert 0.12 < r["frac"] < 0.13


def test_the_eight_rank_forms_of_configs_4_and_5_go_one_level_deeper():
    """`bench.py --gpus 8 --workload raft5 | ssi4x3` searches one BFS level beyond the one-GPU budget (eight
    devices hold it): config 5 against the oracle's 11-level golden, config 4 gated on the oracle's 18 levels with level 19 reported"""
    b = _bench()
    ssi, raft = b.DEEP["ssi4x3"], b.DEEP["raft5"]
    g = json.loads((ROOT / "tests" / "golden" / "ssi_levels.json").read_text())
    c = next(c for c in g["cases"] if c["name"] == ssi["golden"])
    assert ssi["max_levels"] == c["depth"] == 11 and c["distinct"] == 1184049193 and c["verdict"] == "budget"
    assert b.DEEP_TABLE_SLOTS["ssi4x3"] >= 3 * c["distinct"]                      # the sharded tables stay sparse (32-byte probes)
    assert raft["max_levels"] == 19 and raft["golden_prefix"] == 18 and raft["golden"] == "raft5_mcr6_t2_m1_levels18"
    b.WORKLOAD = raft
    G0 = b.golden()
    assert len(G0["prefix_levels"]) == 18 and G0["distinct"] == raft["expect_distinct"] > 924041864
    # --levels L (tests/test_gpu_sharded.py: the same command lines on one shared GPU): a prefix of the same golden, sizes follow
    b.WORKLOAD = dict(raft, max_levels=13, reduced_levels=13)
    G0 = b.golden()
    assert G0["prefix_levels"] == [1, 6, 40, 205, 775, 2851, 10000, 32015, 97215, 287510, 816406, 2225540, 5913945] and G0["distinct"] == sum(G0["prefix_levels"])



def test_dump_outputs_option_writes_the_last_timed_steps_result(tmp_path, monkeypatch, capsys):
    """`bench.py --steps 3 --warmup 2 --dump-outputs DIR` through main(), the engine replaced by a stand-in that returns the golden
    graph with a different queue_left on each call: the dump holds the FIFTH (last timed) call's result, every field float64, exact"""
    import sys
    import numpy as np
    import torch
    import tla_rust_amd as amd
    from tla_rust_amd.binding import Result
    b = _bench()
    g = json.loads((ROOT / "tests" / "golden" / "raft_levels.json").read_text())
    c = next(c for c in g["cases"] if c["name"] == b.WORKLOAD_T3["golden"])
    calls = []

    class StandIn:
        def __init__(self, *args, **kw):
            pass

        def run(self):
            calls.append(len(calls))
            return Result(distinct=c["distinct"], generated=c["generated"], queue_left=len(calls) - 1, depth=c["depth"], verdict="ok",
                          violated_invariant=-1, trace_len=0, levels=list(c["levels"]), seconds=0.125, host_evaluated=False,
                          unchecked_properties=0)

        def kernel_stats(self):
            k = {"launches": 1, "ms_total": 1.0, "units": 1}
            return {"expand": k, "insert": k, "materialise": k, "state_bytes": 136, "cand_cells": 1, "inwave_states": 0}

        def close(self):
            pass

    monkeypatch.setattr(amd, "Engine", StandIn)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    out = tmp_path / "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(out)])
    b.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(calls) == 5 and line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert "cpu_baseline" not in line and "atomic_add" not in line and "pcal" not in line   # (a plain run: those need --full)
    got = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["queue_left"].tolist() == [4.0]                                               # the last timed step's, not a warm-up's
    assert got["depth"].tolist() == [c["depth"]] and got["violated_invariant"].tolist() == [-1.0]
    assert got["distinct"].tolist() == [c["distinct"]] and got["generated"].tolist() == [c["generated"]]
    assert got["level_distinct"].tolist() == c["levels"] and got["verdict"].tolist() == [0.0]


def test_dumped_outputs_are_the_last_steps_result_in_float64(tmp_path):
    """`--dump-outputs DIR`: one float64 array per field of the result the timed call returned, exact for the workload's counts"""
    import numpy as np
    from tla_rust_amd.binding import Result
    b = _bench()
    g = json.loads((ROOT / "tests" / "golden" / "raft_levels.json").read_text())
    c = next(c for c in g["cases"] if c["name"] == b.WORKLOAD_T3["golden"])
    res = Result(distinct=c["distinct"], generated=c["generated"], queue_left=0, depth=c["depth"], verdict="ok", violated_invariant=-1,
                 trace_len=0, levels=list(c["levels"]), seconds=0.125, host_evaluated=False, unchecked_properties=0)
    b.dump_outputs(tmp_path / "out", res)
    got = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert set(got) == {"distinct", "generated", "depth", "queue_left", "verdict", "violated_invariant", "level_distinct"}
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["generated"][0] == c["generated"] and got["distinct"][0] == c["distinct"] == got["level_distinct"].sum()
    assert got["level_distinct"].tolist() == c["levels"] and got["verdict"][0] == 0
    assert got["depth"].tolist() == [c["depth"]] and got["queue_left"].tolist() == [0.0] and got["violated_invariant"].tolist() == [-1.0]
