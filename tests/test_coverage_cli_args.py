"""`mc X.tla -coverage`: what the command line refuses and accepts before it touches a device (no GPU needed)."""
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


@pytest.mark.parametrize("args,other", [
    (["-coverage", "-simulate"], "-simulate"),
    (["-simulate", "num=10", "-coverage"], "-simulate"),
    (["-coverage", "-gpus", "2"], "-gpus"),
    (["-gpus", "2", "-coverage", "5"], "-gpus"),
    (["-coverage", "-recover", "nowhere.ck"], "-recover"),
])
def test_coverage_is_refused_with_simulate_gpus_and_recover(mc, args, other):
    p = subprocess.run([str(mc), str(MODEL), *args], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stderr.strip() == f"mc: -coverage is not available with {other}", (p.returncode, p.stdout, p.stderr)
    assert p.stdout == ""


def test_the_minutes_argument_is_taken(mc):
    """TLC's `-coverage 5`: the number belongs to the option (it is not the module, and not an unknown option); what follows is read on.
    An option mc does not know ends the run with its own message, so reaching it shows that `-coverage 5` was parsed."""
    p = subprocess.run([str(mc), str(MODEL), "-coverage", "5", "-nosuchoption"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "mc: unknown option -nosuchoption" in p.stderr, (p.stdout, p.stderr)
    p = subprocess.run([str(mc), "-coverage", "5"], capture_output=True, text=True, timeout=60)   # no module: "5" was not taken for one
    assert p.returncode == 1 and p.stderr.startswith("usage: mc X.tla"), (p.stdout, p.stderr)
    p = subprocess.run([str(mc), str(MODEL), "-coverage", "-nosuchoption"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "mc: unknown option -nosuchoption" in p.stderr


def test_help_lists_the_option(mc):
    p = subprocess.run([str(mc), "-help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "-coverage" in p.stderr


def test_the_binding_knows_the_flag_and_the_symbol(mc):
    import inspect
    import tla_rust_amd.binding as b
    assert b.MC_F_COVERAGE == 1 << 24 and "coverage" in inspect.signature(b.Engine.__init__).parameters
    assert hasattr(b.lib(), "mc_engine_coverage") and callable(b.Engine.coverage)
    header = (ROOT / "include" / "tlamc.h").read_text()
    assert "#define MC_F_COVERAGE 16777216u" in header
    import ctypes
    assert ctypes.sizeof(b.ActionCoverage) == 24
