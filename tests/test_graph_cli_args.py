"""`mc X.tla -dump dot[,actionlabels][,colorize] FILE` and the state-graph entry points: what the command line refuses and accepts
before it touches a device, and what the binding declares (no GPU needed)."""
import ctypes
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
MC = ROOT / "tla_rust_amd" / "_build" / "mc"
MODEL = ROOT / "specs" / "readme_variant" / "pcal_intro.tla"


@pytest.fixture(scope="module")
def mc():
    import tla_rust_amd.build as b
    b.build()
    return MC


def run(mc, *args):
    return subprocess.run([str(mc), *map(str, args)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,other", [
    (["-dump", "dot", "g.dot", "-simulate"], "-simulate"),
    (["-simulate", "num=10", "-dump", "dot,actionlabels", "g.dot"], "-simulate"),
    (["-dump", "dot,actionlabels,colorize", "g.dot", "-gpus", "2"], "-gpus"),
    (["-gpus", "2", "-dump", "dot", "g.dot"], "-gpus"),
    (["-gpus", "2", "-torch", "-dump", "dot,colorize", "g.dot"], "-gpus"),
])
def test_dump_dot_is_refused_with_simulate_and_gpus(mc, tmp_path, args, other):
    p = subprocess.run([str(mc), str(MODEL), *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 1 and p.stderr.strip() == f"mc: -dump is not available with {other}", (p.returncode, p.stdout, p.stderr)
    assert p.stdout == "" and not (tmp_path / "g.dot").exists()


def test_the_sub_options_and_the_file_name_are_taken(mc):
    """`-dump dot,actionlabels F`: two arguments belong to the option.  An option mc does not know ends the run with its own message,
    so reaching it shows that what stood before it was parsed."""
    for form in ("dot", "dot,actionlabels", "dot,colorize", "dot,actionlabels,colorize", "dot,colorize,actionlabels"):
        p = run(mc, MODEL, "-dump", form, "g.dot", "-nosuchoption")
        assert p.returncode == 1 and "mc: unknown option -nosuchoption" in p.stderr, (form, p.stdout, p.stderr)
    p = run(mc, "-dump", "dot,actionlabels", "g.dot")   # no module: neither argument was taken for one
    assert p.returncode == 1 and p.stderr.startswith("usage: mc X.tla"), (p.stdout, p.stderr)
    p = run(mc, MODEL, "-dump", "dot,actionlabels")     # the file name is missing
    assert p.returncode == 1 and p.stderr.strip() == "mc: -dump dot needs a file name", (p.stdout, p.stderr)
    # plain -dump still takes ONE argument, whatever it is called
    p = run(mc, MODEL, "-dump", "dots", "-nosuchoption")
    assert p.returncode == 1 and "mc: unknown option -nosuchoption" in p.stderr


@pytest.mark.parametrize("form,bad", [("dot,actionlabel", "actionlabel"), ("dot,colorize,snapshot", "snapshot"), ("dot,", "")])
def test_an_unknown_sub_option_is_refused(mc, form, bad):
    p = run(mc, MODEL, "-dump", form, "g.dot")
    assert p.returncode == 1 and p.stderr.rstrip("\n") == f"mc: unknown -dump option {bad}", (p.stdout, p.stderr)
    assert p.stdout == ""


def test_host_evaluated_modules_and_cfgs_without_a_behaviour_are_refused(mc, tmp_path):
    """the existing -dump refusals; both are decided from the module and cfg texts, before an engine is created"""
    (tmp_path / "Tiny.tla").write_text("---- MODULE Tiny ----\nEXTENDS Naturals\nVARIABLE x\nInit == x = 0\nNext == x' = (x + 1) % 3\n====\n")
    (tmp_path / "Tiny.cfg").write_text("INIT Init\nNEXT Next\n")
    p = run(mc, tmp_path / "Tiny.tla", "-dump", "dot", tmp_path / "g.dot")
    assert p.returncode == 1 and "need a GPU lowering (the module is evaluated on the host)" in p.stderr, (p.stdout, p.stderr)
    (tmp_path / "Unit.tla").write_text("---- MODULE Unit ----\nEXTENDS Naturals\nASSUME 1 + 1 = 2\n====\n")
    (tmp_path / "Unit.cfg").write_text("")
    p = run(mc, tmp_path / "Unit.tla", "-dump", "dot,actionlabels", tmp_path / "g.dot")
    assert p.returncode == 1 and "need a behaviour spec" in p.stderr, (p.stdout, p.stderr)
    assert not (tmp_path / "g.dot").exists()


def test_help_lists_the_form(mc):
    p = run(mc, "-help")
    assert p.returncode == 1 and "-dump dot[,actionlabels][,colorize] FILE" in p.stderr and "State k" in p.stderr


def test_the_binding_knows_the_calls_and_the_struct(mc):
    import tla_rust_amd.binding as b
    assert callable(b.Engine.graph) and callable(b.Engine.graph_info)
    for sym in ("mc_engine_graph", "mc_engine_graph_read", "mc_check_files_dot", "mc_check_files_dumps"):
        assert hasattr(b.lib(), sym), sym
    assert len(b.lib().mc_check_files_dot.argtypes) == 8 and len(b.lib().mc_check_files_dumps.argtypes) == 11 and callable(b.check_files_dot)
    assert ctypes.sizeof(b.GraphInfo) == 64
    assert [n for n, _ in b.GraphInfo._fields_] == ["states", "expanded", "init_states", "edges", "self_loops", "dropped", "max_out_degree", "pad", "seconds"]
    header = (ROOT / "include" / "tlamc.h").read_text()
    assert "#define MC_DOT_ACTIONLABELS 1u" in header and "#define MC_DOT_COLORIZE 2u" in header
    assert (b.MC_DOT_ACTIONLABELS, b.MC_DOT_COLORIZE) == (1, 2)
    rust = (ROOT / "bindings" / "rust" / "src" / "lib.rs").read_text()
    assert "pub fn mc_check_files_dot(" in rust and "pub fn mc_check_files_dumps(" in rust
    assert "pub fn mc_engine_graph(" in rust and "pub fn mc_engine_graph_read(" in rust and "pub struct mc_graph_info" in rust
