"""Builds libtlamc.so (HIP kernels + C ABI, gfx950 only) in-tree under tla_rust_amd/_build/.

hipcc cross-compiles without a GPU, so this also runs in the CPU-only dev container."""
import os
import subprocess
from pathlib import Path

PKG = Path(__file__).resolve().parent
CSRC = PKG / "csrc"
OUT = PKG / "_build"
LIB = OUT / "libtlamc.so"
CLI = OUT / "mc"

SOURCES = ["engine.hip", "frontend.cpp"]

# How every device source of the product is compiled.  The test libraries that build the product's kernels outside the product
# (tests/testlib.hip_argv) take the same list; build() adds its environment-driven extras to its own copy only.
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result"]

# What each object of engine.hip depends on: ENGINE_BASE for every unit, ENGINE_OWN[tu] for the lowerings the unit instantiates kernels of
# (engine.hip includes every spec header through spec_registry.h; a unit's code changes only with its own).  state_graph.hip, the host
# half of what consumes the state graph's CSR arrays, is one object for all of them: the spec units never see engine_live.h.
# tests/test_engine_layout.py checks the lists against the files' #include lines.
ENGINE_BASE = ["engine.hip", "hip_owned.h", "engine_kernels.h", "engine_sim.h", "sim_walk.h", "engine_behaviours.h", "behaviour.h", "engine_coverage.h", "coverage.h", "engine_violations.h", "violations.h",
               "engine_graph.h",
               "graph.h", "liveness.h", "live_query.h", "state_graph.h", "spec_gen.h", "mc_common.h", "spec_registry.h", "../../include/tlamc.h"]
ENGINE_OWN = {0: ["spec_pluscal.h", "spec_raft.h", "spec_raft_packed.h", "spec_ssi.h", "spec_vm.h", "spec_vm_cfg.h", "spec_paxos.h", "engine_pairs.h"], 7: ["spec_paxos.h"], 1: ["spec_pluscal.h"],
              2: ["spec_raft.h"], 3: ["spec_raft.h"], 4: ["spec_raft.h"], 5: ["spec_ssi.h", "engine_pairs.h"], 6: ["spec_vm.h", "spec_vm_cfg.h"],
              # raft with 2 / 3 servers over packed rows (spec_raft_packed.h): one unit per instantiation (9 is the unit of generated code, built at load time)
              12: ["spec_raft.h", "spec_raft_packed.h"], 13: ["spec_raft.h", "spec_raft_packed.h"]}
STATE_GRAPH_DEPS = ["state_graph.hip", "state_graph.h", "engine_live.h", "hip_owned.h", "liveness.h", "live_query.h", "graph.h", "coverage.h", "mc_common.h", "spec_registry.h",
                    "spec_gen.h", "spec_pluscal.h", "spec_raft.h", "spec_raft_packed.h", "spec_ssi.h", "spec_vm.h", "spec_vm_cfg.h", "spec_paxos.h", "../../include/tlamc.h"]


def _stale(target, deps):
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(d.stat().st_mtime > t for d in deps)


def build(force=False, verbose=False):
    OUT.mkdir(exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    deps = list(CSRC.glob("*")) + [PKG.parent / "include" / "tlamc.h"]
    srcs = [str(CSRC / s) for s in SOURCES if (CSRC / s).exists()]
    # engine.hip is compiled once per group of specs (MC_TU = 1..7) plus once for the C ABI (MC_TU = 0), in
    # parallel: the unrolled per-spec kernels dominate compile time.  Each object is rebuilt only when one of the
    # files it really depends on changed (a TU instantiates the kernels of its own spec header only).
    common = [hipcc] + HIP_FLAGS + ["-I", str(PKG.parent / "include")]
    if os.environ.get("TLAMC_LINE_TABLES"):  # source lines for rocprofv3's PC sampling (profiles/pcsample.sh); code generation unchanged
        common.append("-gline-tables-only")
    if os.environ.get("TLAMC_EXTRA_DEFS"):   # A/B builds: extra -D flags (e.g. -DMC_NT_PARENT), space-separated
        common += os.environ["TLAMC_EXTRA_DEFS"].split()
    if os.environ.get("TLAMC_PHASE_PROF"):   # per-phase cycle counters inside k_expand_family (profiles/phase_prof.py): a profiling build
        common.append("-DMC_PHASE_PROF")
    jobs, objs = [], []
    for tu in sorted(ENGINE_OWN):
        obj = OUT / f"engine_tu{tu}.o"
        objs.append(obj)
        if force or _stale(obj, [CSRC / h for h in ENGINE_BASE + ENGINE_OWN[tu]]):
            jobs.append((obj, subprocess.Popen(common + ["-x", "hip", f"-DMC_TU={tu}", "-c", str(CSRC / "engine.hip"), "-o", str(obj)])))
    # the state graph's consumers (SCC, fairness, reads) and the device scans: one object, whatever the lowering
    obj = OUT / "state_graph.o"
    objs.append(obj)
    if force or _stale(obj, [CSRC / d for d in STATE_GRAPH_DEPS]):
        jobs.append((obj, subprocess.Popen(common + ["-x", "hip", "-c", str(CSRC / "state_graph.hip"), "-o", str(obj)])))
    host_deps = {"frontend": ["frontend.cpp", "pcal.h", "spec_vm.h", "mc_common.h", "tlaeval.h"], "pcal": ["pcal.cpp", "pcal.h"],
                 "tlaeval": ["tlaeval.cpp", "tlaeval.h"],
                 "pcal_compile": ["pcal_compile.cpp", "pcal.h", "spec_vm.h", "spec_vm_cfg.h", "mc_common.h"],
                 "pcal_codegen": ["pcal_codegen.cpp", "pcal.h", "spec_vm.h", "mc_common.h"]}
    for name, dd in host_deps.items():
        obj = OUT / f"{name}.o"
        objs.append(obj)
        if force or _stale(obj, [CSRC / d for d in dd] + [PKG.parent / "include" / "tlamc.h"]):
            jobs.append((obj, subprocess.Popen(common + ["-x", "hip", "-c", str(CSRC / f"{name}.cpp"), "-o", str(obj)])))
    # the hip-rccl back-end: host code over the public C ABI, HIP runtime and RCCL
    obj = OUT / "shard_rccl.o"
    objs.append(obj)
    if force or _stale(obj, [CSRC / "shard_rccl.cpp", CSRC / "shard_loop.h", PKG.parent / "include" / "tlamc.h"]):
        jobs.append((obj, subprocess.Popen(common + ["-x", "hip", "-c", str(CSRC / "shard_rccl.cpp"), "-o", str(obj)])))
    for obj, pr in jobs:
        if pr.wait() != 0:
            raise RuntimeError(f"hipcc failed for {obj.name}")
    if force or jobs or not LIB.exists():
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(LIB)] + [str(o) for o in objs] + ["-ldl", "-pthread"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    main = CSRC / "mc_main.cpp"
    if main.exists() and (force or _stale(CLI, deps + [LIB])):
        cmd = [hipcc, "-O2", "-std=c++17", "-I", str(PKG.parent / "include"), "-o", str(CLI), str(main),
               "-L", str(OUT), "-ltlamc", "-Wl,-rpath,$ORIGIN"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    # profiling aid, not part of the product: known-byte access patterns to calibrate rocprofv3's FETCH_SIZE / WRITE_SIZE (profiles/calib)
    calib_src = PKG.parent / "profiles" / "calib" / "calib_fetch.hip"
    calib = OUT / "calib_fetch"
    if calib_src.exists() and (force or _stale(calib, [calib_src])):
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-Wno-unused-value", "-Wno-unused-result", "-o", str(calib), str(calib_src)], check=True)
    # ... and the random-probe rate against the working set / the cost of partitioning candidates by table region (profiles/calib/probe_locality.hip)
    loc_src = PKG.parent / "profiles" / "calib" / "probe_locality.hip"
    loc = OUT / "probe_locality"
    if loc_src.exists() and (force or _stale(loc, [loc_src])):
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-Wno-unused-value", "-Wno-unused-result", "-o", str(loc), str(loc_src)], check=True)
    return LIB


if __name__ == "__main__":
    print(build(force=True, verbose=True))
