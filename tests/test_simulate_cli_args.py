"""`mc` refuses malformed simulation options before it touches a device (no GPU needed): -depth / -seed only with -simulate, and
numbers that are whole numbers."""
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


@pytest.mark.parametrize("args,msg", [
    (["-depth", "5"], "-depth needs -simulate"),
    (["-seed", "3"], "-seed needs -simulate"),
    (["-simulate", "-seed", "abc"], "-seed needs a non-negative integer"),
    (["-simulate", "-seed", "-1"], "-seed needs a non-negative integer"),
    (["-simulate", "-seed", "12x"], "-seed needs a non-negative integer"),
    (["-simulate", "-depth", "0"], "-depth needs a number of states"),
    (["-simulate", "-depth", "ten"], "-depth needs a number of states"),
    (["-simulate", "num=0"], "num=N needs a number of walks"),
    (["-simulate", "num=5k"], "num=N needs a number of walks"),
    (["-simulate", "num=1099511627777"], "num=N needs a number of walks"),
])
def test_malformed_simulation_options_are_refused(mc, args, msg):
    p = subprocess.run([str(mc), str(MODEL), *args], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and msg in p.stderr, (p.returncode, p.stdout, p.stderr)
