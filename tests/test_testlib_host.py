"""tests/testlib.py itself, on the host: the builder on a three-line C source (built when stale, once for all who ask together, nothing
left behind by a compile that fails) and the maker of mutant trees (the product's headers with exactly one replacement)."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import testlib


@pytest.fixture
def lib(tmp_path):
    """(so, argv, deps, runs): a library of one C source; argv[0] is a wrapper that counts its runs before it starts the compiler"""
    src, log = tmp_path / "three.c", tmp_path / "runs"
    src.write_text("int three(void) {\n    return 3;\n}\n")
    log.write_text("")
    cc = tmp_path / "cc"
    cc.write_text(f'#!/bin/sh\necho run >> "{log}"\nexec gcc "$@"\n')
    cc.chmod(0o755)
    return tmp_path / "out" / "libthree.so", [cc, "-shared", "-fPIC", src], [src], lambda: len(log.read_text().splitlines())


def older(path, seconds):
    t = path.stat().st_mtime - seconds
    os.utime(path, (t, t))


def test_a_fresh_library_is_not_built_again_and_a_touched_dep_rebuilds_it(lib):
    so, argv, deps, runs = lib
    assert testlib.build_library(so, argv, deps) == so and so.exists() and runs() == 1   # (the output directory is made)
    older(so, 10)   # (both into the past, the library still the newer one: a rebuild shows in its time)
    older(deps[0], 100)
    before = so.stat().st_mtime
    assert testlib.build_library(so, argv, deps) == so and so.stat().st_mtime == before and runs() == 1
    os.utime(deps[0])
    assert testlib.build_library(so, argv, deps) == so and so.stat().st_mtime > before and runs() == 2
    assert sorted(p.name for p in so.parent.iterdir()) == [".lock", "libthree.so"]   # no temporary name is left


def test_four_threads_compile_a_stale_library_once(lib):
    so, argv, deps, runs = lib
    with ThreadPoolExecutor(4) as pool:
        assert list(pool.map(lambda _: testlib.build_library(so, argv, deps), range(4))) == [so] * 4
    assert runs() == 1 and so.exists()


def test_a_compile_that_fails_raises_and_leaves_no_library(lib):
    so, argv, deps, runs = lib
    deps[0].write_text("int three(void) { return }\n")
    with pytest.raises(subprocess.CalledProcessError):
        testlib.build_library(so, argv, deps)
    assert runs() == 1 and not so.exists()
    # ... and the next who asks compiles again
    deps[0].write_text("int three(void) { return 3; }\n")
    assert testlib.build_library(so, argv, deps).exists() and runs() == 2


def test_the_argument_lists():
    hip = testlib.hip_argv("-I", "x", "a.hip")
    assert hip[0] == os.environ.get("HIPCC", "/opt/rocm/bin/hipcc") and hip[-6:] == ["-shared", "-x", "hip", "-I", "x", "a.hip"]
    import tla_rust_amd.build as product
    assert hip[1:-6] == product.HIP_FLAGS and product.HIP_FLAGS[0].endswith("=gfx950") and "-O3" in product.HIP_FLAGS   # the product's, whatever they are
    assert testlib.host_argv("-O2", "a.cpp") == ["g++", "-std=c++17", "-fPIC", "-shared", "-O2", "a.cpp"]
    deps = testlib.product_deps(testlib.CSRC)
    assert testlib.ROOT / "include" / "tlamc.h" in deps and testlib.CSRC / "graph.h" in deps and all(d.suffix == ".h" for d in deps)


ONCE = "constexpr uint64_t GRAPH_ABSENT = ~0ull;"   # a text graph.h holds once, and one it holds several times
TWICE = "GRAPH_ABSENT"


def test_mutant_tree_refuses_an_edit_that_is_not_one_replacement(tmp_path):
    text = (testlib.CSRC / "graph.h").read_text()
    assert text.count(ONCE) == 1 and text.count(TWICE) >= 2
    for old, new in (("no such text in graph.h", "x"), (TWICE, "x"), (ONCE, ONCE)):
        with pytest.raises(AssertionError):
            testlib.mutant_tree(tmp_path, "refused", ("graph.h", old, new))
    with pytest.raises(AssertionError):   # the second of a list is checked like the first
        testlib.mutant_tree(tmp_path, "refused", [("graph.h", ONCE, "constexpr uint64_t GRAPH_ABSENT = 0;"), ("graph.h", ONCE, "x")])


def test_mutant_tree_differs_from_the_product_in_the_one_replacement_and_keeps_its_times(tmp_path):
    new = "constexpr uint64_t GRAPH_ABSENT = 0;"
    d = testlib.mutant_tree(tmp_path, "m", ("graph.h", ONCE, new), also=["state_graph.hip"])
    assert d == tmp_path / "m" / "tla_rust_amd" / "csrc"
    want = {f.name for f in testlib.CSRC.glob("*.h")} | {"state_graph.hip"}
    assert {f.name for f in d.iterdir()} == want and [f.name for f in (tmp_path / "m" / "include").iterdir()] == ["tlamc.h"]
    for name in want - {"graph.h"}:
        assert (d / name).read_bytes() == (testlib.CSRC / name).read_bytes(), name
    assert (tmp_path / "m" / "include" / "tlamc.h").read_bytes() == (testlib.ROOT / "include" / "tlamc.h").read_bytes()
    assert (d / "graph.h").read_text() == (testlib.CSRC / "graph.h").read_text().replace(ONCE, new) != (testlib.CSRC / "graph.h").read_text()
    assert testlib.product_deps(d)[-1] == tmp_path / "m" / "include" / "tlamc.h"
    files = [*d.iterdir(), tmp_path / "m" / "include" / "tlamc.h"]
    for f in files:
        older(f, 50)
    times = {f: f.stat().st_mtime_ns for f in files}
    assert testlib.mutant_tree(tmp_path, "m", ("graph.h", ONCE, new), also=["state_graph.hip"]) == d
    assert {f: f.stat().st_mtime_ns for f in files} == times


def test_build_mutants_and_survives():
    assert list(testlib.build_mutants(["b", "a", "c"], str.upper).items()) == [("b", "B"), ("a", "A"), ("c", "C")]

    def fails():
        assert False
    assert testlib.survives(lambda: None) and not testlib.survives(fails)
    with pytest.raises(ValueError):   # an error of another kind is no verdict on the mutant
        testlib.survives(lambda: int("x"))
