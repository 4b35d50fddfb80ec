"""What every test library under tests/_*/ shares: the one builder (compile when stale, under a lock, into a temporary name) with the
product's own flags for device code, and the one maker of mutant trees (a copy of the product's sources with one text replaced)."""
import fcntl
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "tla_rust_amd" / "csrc"


# ------------------------------------------------------------------------------------------------ the builder
def build_library(so, argv, deps):
    """`so`, built with argv + ["-o", a temporary name] when it is missing or older than one of `deps`.  Several ranks of a multi-process
    test, or several workers of one run, may arrive here together: one builds and renames the complete file into place, the others
    wait for the lock on the directory and find the library fresh."""
    def fresh():
        return so.exists() and all(so.stat().st_mtime >= d.stat().st_mtime for d in deps)
    if fresh():
        return so
    so.parent.mkdir(parents=True, exist_ok=True)
    with open(so.parent / ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not fresh():
            tmp = so.parent / f"{so.stem}.{os.getpid()}.so"
            subprocess.run([str(a) for a in argv] + ["-o", str(tmp)], check=True)
            os.replace(tmp, so)
    return so


def hip_argv(*more):
    """device code for gfx950, compiled the way the product's is (tla_rust_amd/build.py: HIP_FLAGS)"""
    from tla_rust_amd.build import HIP_FLAGS   # (here: helpers imports this module in scripts that have tests/ alone on their path)
    return [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + HIP_FLAGS + ["-shared", "-x", "hip", *more]


def host_argv(*more):
    return ["g++", "-std=c++17", "-fPIC", "-shared", *more]


def product_deps(csrc):
    """the headers of a csrc directory and the include/tlamc.h that belongs to it (the product's headers include ../../include/tlamc.h:
    a copy of csrc brings its own)"""
    return sorted(csrc.glob("*.h")) + [csrc.parent.parent / "include" / "tlamc.h"]


def build_generated(so, hdr, text, more):
    """a harness compiled around the generated code `text` (its GEN_HEADER).  The caller keys `so` and `hdr` by a hash of everything
    the library is made of, so the library is built when it is missing and never goes stale."""
    hdr.parent.mkdir(parents=True, exist_ok=True)
    write_if_changed(hdr, text)
    return build_library(so, host_argv("-O1", "-w", "-I", CSRC, "-I", ROOT / "include", f'-DGEN_HEADER="{hdr}"', *more), [])


# ------------------------------------------------------------------------------------------------ mutants
def write_if_changed(path, text):
    if not path.exists() or path.read_text() != text:   # (an unchanged copy keeps its time: the library built from it stays fresh)
        path.write_text(text)


FRONT_END = ("pcal.cpp", "pcal_compile.cpp", "pcal_codegen.cpp")   # the PlusCal front end: host code that some libraries compile in


def mutant_texts(edits, also=()):
    """{file name: text} of the product's headers and the sources `also` names (the product's by name, a test's own source by its path),
    with one (file, old, new) or a list of them applied.  Every `old` must occur exactly once and differ from its `new`."""
    if edits and isinstance(edits[0], str):
        edits = [edits]
    texts = {f.name: f.read_text() for f in [*CSRC.glob("*.h"), *(CSRC / a for a in also)]}
    for file, old, new in edits:
        assert texts[file].count(old) == 1 and old != new, (file, old)
        texts[file] = texts[file].replace(old, new)
    return texts


def mutant_tree(top, name, edits, also=()):
    """top/name/tla_rust_amd/csrc holding mutant_texts(edits, also), and top/name/include/tlamc.h where those headers look for it.  A
    file that is there unchanged is not written again.  Returns the csrc directory."""
    d = top / name / "tla_rust_amd" / "csrc"
    d.mkdir(parents=True, exist_ok=True)
    (top / name / "include").mkdir(exist_ok=True)
    for file, text in mutant_texts(edits, also).items():
        write_if_changed(d / file, text)
    write_if_changed(top / name / "include" / "tlamc.h", (ROOT / "include" / "tlamc.h").read_text())
    return d


def build_mutants(names, build_one):
    """{name: build_one(name)} in the order of `names`, built side by side (the threads wait for one compiler each)"""
    names = list(names)
    with ThreadPoolExecutor(len(names)) as pool:
        return dict(zip(names, pool.map(build_one, names)))


def survives(fn):
    """does the comparison `fn` pass?  (a mutant is killed when it does not)"""
    try:
        fn()
    except AssertionError:
        return False
    return True
