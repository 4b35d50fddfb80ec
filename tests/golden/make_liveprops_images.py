"""Writes tests/golden/liveprops_images.json: per cfg under specs/pluscal and specs_liveness, the SHA-256 of what the front end compiles
it to — program image, the scalar fields of VmParams, generated header (null: a cfg the compiler refuses).  The committed file was
written by the front end as it was BEFORE it knew the temporal properties of DESIGN section 17 (with the image read by the same few
lines as tests/_livepropshim's livepropshim_image); tests/test_liveprops_host.py asserts that a cfg which names no such property still
compiles to exactly that.  Run it again only when the compiled form of these programs is meant to change.

    python tests/golden/make_liveprops_images.py"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import tla_rust_amd as amd  # noqa: E402
import test_liveprops_host as t  # noqa: E402

out = {}
for tla, cfg in t.old_cfgs():
    key = str(cfg.relative_to(ROOT))
    try:
        p = amd.Program(tla.read_text(), cfg.read_text())
    except amd.McError:
        out[key] = None
        continue
    image, fields = t.image_of(p)
    out[key] = t.digest(image, fields, t.header_of(amd, p))
    p.close()
t.GOLDEN.write_text(json.dumps(out, indent=1, sort_keys=True))
print(len(out), "cfgs")
