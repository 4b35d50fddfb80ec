"""spec_raft_packed.h against spec_raft.h on the host (CPU only): tests/_packshim/packshim.cpp builds both headers without HIP and runs
SpecRaft<3> and SpecRaftPacked<3> in lockstep.  For every (state, slot) it meets, the program itself checks — and stops at the first
difference — that the status bits and the successor's fingerprint are equal, that export_row(packed successor) is the base's successor
byte for byte (for apply, apply_known_fp and the in-wave writer apply_summary_patch), and that the incrementally kept fingerprint equals
the full recomputation; besides: load / load_expand give the same Summary and Guards, eval_pair and eval_dense the same results.

The states come from three runs, each module-scoped and run once:
  bfs     the complete graph raft3_mcr4_t2_m1_k5_complete (178 654 states), with the slot-array capacities 10 / 1 / 4 of the bench rows;
  walk    fixed-seed random walks under the t3 parameters of bench.py's workload;
  script  scripted behaviours under the t3 constants with MaxMsgKeys 16: a second election by servers that hold a log needs more than
          the 8 message keys the t3 model allows (4 for the first election, 2 per replicated entry, 2 per vote), and no random walk of
          useful length gets there (the walk run reports what it reached).
The coverage the issue asks for is asserted on what the runs report, never assumed."""
import json
import subprocess
from pathlib import Path

import pytest

import testlib

ROOT = Path(__file__).resolve().parent.parent
DIR = ROOT / "tests" / "_packshim"
CSRC = ROOT / "tla_rust_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden" / "raft_levels.json"
K5 = [3, 4, 2, 3, 1, 1, 10, 1, 4, 5]      # raft3_mcr4_t2_m1_k5_complete (MaxMsgKeys 5) in rows of 16 words / 13 packed
T3 = [3, 4, 3, 3, 1, 1, 8, 2, 4, 8]       # bench.py's default workload: 17 words / 13 packed
T3_KEYS16 = [3, 4, 3, 3, 1, 1, 16, 2, 4, 16]


def build():
    return testlib.build_library(DIR / "_build" / "packshim", ["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", DIR / "packshim.cpp"],
                                 [DIR / "packshim.cpp", CSRC / "spec_raft.h", CSRC / "spec_raft_packed.h", CSRC / "mc_common.h"])


def run(*args):
    p = subprocess.run([str(build())] + [str(a) for a in args], capture_output=True, text=True)
    assert p.returncode == 0, (args, p.stderr)
    return json.loads(p.stdout)


@pytest.fixture(scope="module")
def bfs():
    return run("bfs", *K5)


@pytest.fixture(scope="module")
def walk():
    return run("walk", 1, 2000, 80, *T3)


@pytest.fixture(scope="module")
def script():
    return run("script", *T3_KEYS16)


def test_k5_complete_graph_in_lockstep(bfs):
    c = next(c for c in json.loads(GOLDEN.read_text())["cases"] if c["name"] == "raft3_mcr4_t2_m1_k5_complete")
    assert bfs["words"] == [16, 13]
    assert bfs["levels"] == c["levels"] and bfs["distinct"] == c["distinct"] == bfs["states"]
    assert bfs["generated"] + 1 == c["generated"]          # (the golden counts the initial state)
    assert all(n > 0 for n in bfs["classes"]) and len(bfs["classes"]) == 10
    assert bfs["successors"] > 900_000 and bfs["eadd"] > 0


def test_t3_walks_in_lockstep(walk):
    assert walk["words"] == [17, 13]
    assert walk["states"] > 50_000 and walk["successors"] > 300_000
    assert all(n > 0 for n in walk["classes"]) and len(walk["classes"]) == 10
    assert walk["eadd"] > 0


def test_second_elections_with_logs_in_lockstep(script):
    assert script["words"] == [21, 17]
    assert all(n > 0 for n in script["classes"])


def test_the_runs_cover_what_packing_touches(bfs, walk, script):
    runs = (bfs, walk, script)
    for k in range(10):                                      # all 10 slot classes fired
        assert sum(r["classes"][k] for r in runs) > 0, k
    for e in range(9):                                       # every voterLog entry (i, j) was non-zero in some state
        assert sum(r["voterlog"][e] for r in runs) > 0, divmod(e, 3)
    assert sum(r["two_elections"] for r in runs) > 0         # some state held two election records
    assert sum(r["clear_between"] for r in runs) > 0         # a vmode 1 clear on a server whose neighbours' fields were non-zero
    assert sum(r["vset"] for r in runs) > 0                  # a vmode 2 set of a non-empty log
    assert script["clear_between"] > 0 and script["two_elections"] > 0 and min(script["voterlog"]) > 0


def test_packable_by_log_width():
    assert run("packable") == {"2": True, "3": True, "4": True, "6": True, "8": False, "9": False, "10": False}


def test_a_full_entry_stays_in_its_field():
    """lb = 6: entry (2, 2) — the topmost of the voterLog word, bits [48, 54) — set to all ones, by import_row and by the writer"""
    r = run("field")
    assert r == {"placed": True, "bit54_and_above_clear": True, "round_trip": True, "writer": True, "other_words_kept": True, "election_word": True}


def test_public_rows_keep_their_width():
    """what the C ABI hands out does not change: mc_state_bytes of the raft rows (the packed width is an engine's own)"""
    text = (CSRC / "spec_registry.h").read_text()
    assert "return f(SpecRaft2{}, p);" in text and "return f(SpecRaft3{}, p);" in text and "SpecRaftPacked" not in text.split("dispatch_spec(")[1]
