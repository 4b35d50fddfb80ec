"""libtlamc.so loads and exports every symbol include/tlamc.h declares (no compute calls: CPU only)."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_every_declared_symbol_is_exported():
    import tla_rust_amd.build as b
    so = b.build()
    lib = ctypes.CDLL(str(so))
    header = (ROOT / "include" / "tlamc.h").read_text()
    names = set(re.findall(r"\b(mc_[a-z_]+)\s*\(", header))
    assert len(names) >= 25
    missing = [n for n in sorted(names) if not hasattr(lib, n)]
    assert not missing, missing


def test_no_cpu_fallback_without_a_device():
    """The product path must fail loudly without a GPU (and never route through the oracle).  Run in a child process: the probe
    initialises the HIP runtime, which in a container without /dev/kfd leaves runtime threads behind — the long-lived pytest
    process (two sporadic segfaults with no Python frame in five full-suite runs) should not carry them."""
    import subprocess
    import sys
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import tla_rust_amd as amd\n"
        "if amd.device_count() > 0:\n"
        "    print('HAS_DEVICE'); raise SystemExit(0)\n"
        "try:\n"
        "    amd.Engine('atomic_add', [3])\n"
        "except amd.McError as e:\n"
        "    print('REFUSED', e.code, 'no CPU fallback' in str(e))\n"
        "else:\n"
        "    print('CREATED')\n" % str(ROOT))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    out = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else p.stderr[-500:]
    assert out == "HAS_DEVICE" or out == "REFUSED -2 True", (out, p.stderr[-500:])


def test_product_does_not_reference_the_oracle():
    for p in list((ROOT / "tla_rust_amd").rglob("*.py")) + list((ROOT / "tla_rust_amd" / "csrc").glob("*")):
        if p.is_file() and p.suffix in (".py", ".h", ".hip", ".cpp"):
            assert "oracle/" not in p.read_text().replace("oracle/spec_raft.c:raft_print", ""), p


def test_route_overflows_are_error_codes_not_words():
    """A round with more candidates than a route bucket / the slot's pending list holds is MC_EROUTE from the engine itself (the level
    loop restarts with twice the allowance); nothing above the C ABI looks at the words of an error message"""
    root = Path(__file__).resolve().parent.parent / "tla_rust_amd" / "csrc"
    engine, kernels, ops, loop = ((root / f).read_text() for f in ("engine.hip", "engine_kernels.h", "shard_rccl.cpp", "shard_loop.h"))
    assert "strstr(" not in ops and "strstr(" not in loop and "mc_last_error()" not in loop
    at = engine.index("slot's pending list holds")
    assert "return MC_EROUTE" in engine[at:at + 120]
    assert kernels.count("err |= DEV_EROUTE;") == 2   # the route sub-buckets of both expand kernels


def test_the_counter_stamp_covers_device_code_only():
    """the kernels live in engine_kernels.h, the host half (Engine, C ABI, checkpoints) in engine.hip; the stamp
    of a counter collection hashes the former (+ the spec lowering and mc_common.h), so a host-side fix does not invalidate counters"""
    import importlib.util
    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("bench_module2", root / "bench.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    src = (root / "bench.py").read_text()
    assert all("engine_kernels.h" in v and "mc_common.h" in v for v in b.KERNEL_SOURCES.values()) and "engine_pairs.h" in b.KERNEL_SOURCES["ssi"]
    assert "engine_pairs.h" not in b.KERNEL_SOURCES["raft"]   # (the by-pairs kernel has its own file: the raft stamp does not move with it)
    assert len({b.kernel_source_hash(k) for k in b.KERNEL_SOURCES}) == len(b.KERNEL_SOURCES)
    assert "engine_kernels.h" in (root / "profiles" / "summarize_pmc.py").read_text()
    host, dev = (root / "tla_rust_amd" / "csrc" / "engine.hip").read_text(), (root / "tla_rust_amd" / "csrc" / "engine_kernels.h").read_text()
    assert "__global__" not in host, "a kernel in the host half"
    assert "__global__" not in (root / "tla_rust_amd" / "csrc" / "state_graph.hip").read_text(), "a kernel in the host half of the graph passes"
    assert "hipMalloc" not in dev and "struct Engine" not in dev and len(b.kernel_source_hash()) == 16
