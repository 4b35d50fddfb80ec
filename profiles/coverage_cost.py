"""What MC_F_COVERAGE costs: the search time (mc_result.seconds, clock started after the tables are cleared) of one model on one
library, several runs in one process after one warm-up run.  One JSON line per (library, model, configuration).

    python profiles/coverage_cost.py LABEL [raft_t3] [pagecache_jit] [--runs N]

$TLAMC_TREE names the tree whose tla_rust_amd package (binding + built library) is measured, this one by default; run it once per
tree — a built checkout of the parent commit (the coverage configuration is skipped where the binding has none) and this one — and
compare the lines (DESIGN.md section 14 says what has been measured so far)."""
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, os.environ.get("TLAMC_TREE") or str(ROOT))
import tla_rust_amd as amd  # noqa: E402

label = sys.argv[1]
models = [a for a in sys.argv[2:] if not a.startswith("--") and not a.isdigit()] or ["raft_t3", "pagecache_jit"]
runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 5
has_cov = "coverage" in amd.Engine.__init__.__code__.co_varnames


def measure(name, spec, params, expect, **kw):
    configs = [("trace off", dict(trace=False)), ("trace on", dict(trace=True))] + ([("coverage", dict(coverage=True))] if has_cov else [])
    for cname, ckw in configs:
        eng = amd.Engine(spec, params, **kw, **ckw)
        r = eng.run()   # warm-up: code objects loaded, memory touched
        assert (r.distinct, r.generated, r.verdict) == expect, (r.distinct, r.generated, r.verdict)
        secs = []
        for _ in range(runs):
            r = eng.run()
            secs.append(r.seconds)
        line = dict(library=label, model=name, config=cname, runs=runs, seconds=[round(s, 5) for s in secs], median=round(statistics.median(secs), 5),
                    min=round(min(secs), 5), max=round(max(secs), 5), distinct=r.distinct, generated=r.generated)
        if cname == "coverage":
            cov = eng.coverage()
            assert sum(n for _, n in cov.values()) == r.generated and sum(d for d, _ in cov.values()) == r.distinct
            line["coverage"] = {k: list(v) for k, v in cov.items()}
        eng.close()
        print(json.dumps(line), flush=True)


if "raft_t3" in models:   # bench.py's workload: specs/MCraft_t3.cfg, the complete graph
    measure("raft MCraft_t3.cfg", "raft", [3, 4, 3, 3, 1, 1, 8, 2, 4, 8], (525782408, 6708500293, "ok"),
            table_capacity=40 << 26, arena_capacity=525782408 + (1 << 20), chunk_states=(1 << 24) - 256)   # (bench.py's capacities)
if "pagecache_jit" in models:   # specs/pluscal/pagecache.tla N = 3 as generated code (-jit)
    prog = amd.Program((ROOT / "specs" / "pluscal" / "pagecache.tla").read_text(), "CONSTANTS N = 3 Blind = FALSE\nINVARIANTS Conservation HeadIsAllocated\n")
    measure("pagecache.tla N=3 -jit", "pcal", prog.params, (20254597, 47629297, "ok"), jit=True, table_capacity=1 << 27, arena_capacity=22 << 20,
            chunk_states=1 << 21)
    prog.close()
