"""Child process of tests/test_gpu_seenset_load.py: searches with the engine in a process of its own, because the engine reads
TLAMC_SPARSE_RATIO once per process.  python tests/seen_load_worker.py '<json: a list of {spec, params, kw}>' prints one JSON line: per
run the result's counts and the seen-set's form (mc_engine_seen_layout), or the error code."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import tla_rust_amd as amd  # noqa: E402


def main():
    out = []
    for job in json.loads(sys.argv[1]):
        eng = amd.Engine(job["spec"], job["params"], **job["kw"])
        try:
            r = eng.run()
            out.append(dict({k: r[k] for k in ("distinct", "generated", "depth", "verdict", "levels")}, layout=list(eng.seen_layout())))
        except amd.McError as e:
            out.append(dict(error=e.code, what=str(e)))
        finally:
            eng.close()
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
