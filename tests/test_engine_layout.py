"""Where the code of the library lives (CPU only): the passes over the state graph's CSR arrays (state_graph.hip + engine_live.h: reads,
components, the fairness check, the device scans) are ONE object, and the per-lowering units of engine.hip — and with them the unit of
generated code built at load time — hold none of it; the dependency lists of the build and the cache key of that load-time build cover
every file the units include."""
import importlib.util
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "tla_rust_amd" / "csrc"
SHARED = re.compile(r"k_scc_|k_live_(indegree|tfill|reduce|verdict)|DeviceScan")
# bench.py's stamps of the kernel sources at the commit before the graph passes moved: the move touches no file they hash
STAMPS = {"raft": "265edb300aeecb16", "ssi": "16ef3e5853ce6d39", "vm": "16190a0edd3e36be"}


def symbols(obj):
    return subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout.splitlines()


def test_the_graph_passes_are_one_object():
    import tla_rust_amd.build as b
    b.build()
    for tu in range(1, 8):
        hits = [ln for ln in symbols(b.OUT / f"engine_tu{tu}.o") if SHARED.search(ln)]
        assert not hits, (tu, hits[:3])
    shared = [ln for ln in symbols(b.OUT / "state_graph.o") if SHARED.search(ln)]
    for name in ("k_scc_trim", "k_scc_colour", "k_scc_back", "k_scc_stats", "k_live_indegree", "k_live_tfill", "k_live_reduce", "k_live_verdict", "DeviceScan"):
        assert any(name in ln for ln in shared), name


def test_the_host_halves_hold_no_kernel_and_no_scan():
    for f in ("engine.hip", "state_graph.hip"):
        text = (CSRC / f).read_text()
        assert "__global__" not in text and "hipcub" not in text, f
    live = (CSRC / "engine_live.h").read_text()
    assert "__global__" in live and "hipcub" in live and "engine_kernels.h\"" not in live
    assert '#include "engine_live.h"' not in (CSRC / "engine.hip").read_text()


def includes(start):
    """the files `start` reaches through #include "..." lines (MC_GEN_HEADER is a macro, not a quoted name: the generated header is
    hashed by its text), as paths relative to csrc"""
    seen, todo = set(), [CSRC / start]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read_text(), flags=re.M):
            g = (f.parent / name).resolve()
            assert g.exists(), (f.name, name)
            todo.append(g)
    return seen


def test_the_source_lists_cover_what_the_units_include():
    import tla_rust_amd.build as b
    engine, graph = includes("engine.hip"), includes("state_graph.hip")
    assert CSRC / "state_graph.h" in engine and CSRC / "engine_live.h" in graph and CSRC / "engine_live.h" not in engine
    assert CSRC / "engine_kernels.h" not in graph
    listed = {(CSRC / f).resolve() for f in b.ENGINE_BASE} | {(CSRC / f).resolve() for own in b.ENGINE_OWN.values() for f in own}
    assert engine <= listed, sorted(p.name for p in engine - listed)
    assert "engine_live.h" not in b.ENGINE_BASE
    assert graph <= {(CSRC / f).resolve() for f in b.STATE_GRAPH_DEPS}, sorted(p.name for p in graph - {(CSRC / f).resolve() for f in b.STATE_GRAPH_DEPS})
    # the load-time build of generated code keys its cache by a listing of csrc (*.h, *.hip) and the public header: every file of
    # the unit is one of those, and the key is no hand-kept list of names
    tlamc = (ROOT / "include" / "tlamc.h").resolve()
    for f in engine:
        assert f == tlamc or (f.parent == CSRC.resolve() and f.suffix in (".h", ".hip")), f
    codegen = (CSRC / "pcal_codegen.cpp").read_text()
    key = codegen[codegen.index("uint64_t h = fnv(gen);"):codegen.index('getenv("TLAMC_JIT_DEFS")')]
    assert "readdir(" in key and '".h"' in key and '".hip"' in key and '"/tlamc.h"' in key
    assert not re.search(r'"/\w+\.(h|hip)"', key.replace('"/tlamc.h"', "")), "a file named by hand in the cache key"


def test_the_kernel_stamps_did_not_move():
    spec = importlib.util.spec_from_file_location("bench_module3", ROOT / "bench.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert {k: b.kernel_source_hash(k) for k in STAMPS} == STAMPS
