#!/usr/bin/env python3
"""Put one MI355X run of tests/test_gpu_normal_render.py on file.  usage: record_normal_render_margins.py LOG

LOG is the output of `pytest -s -m gpu tests/test_gpu_normal_render.py`.  Its NORMAL_RENDER_ROW lines become
profiles/normal_render/margins.jsonl as they are, and per frame the E_kernel of the backward (per output) and of the forward the
"E_kernel" entry of tests/golden/normal_render_margins.json -- a record only: no test reads it as a bound.  "E_f32" and "floor" (the
float32 restatement's errors on the CPU matrix, tests/test_normal_render_reference.py holds them) are left as they are.  A log without
a row of every kind the tests print, or without a forward and a backward row for every frame, is refused and nothing is written."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "NORMAL_RENDER_ROW "
EXPECTED = ("gaussian_normals", "gaussian_normals_backward", "forward", "backward", "cross_features_backward", "cross_existing_backward", "linear",
            "consistency", "trainer")


def main(log):
    with open(log) as f:
        rows = [json.loads(l[l.index(TAG) + len(TAG):]) for l in f if TAG in l]      # (anywhere in a line: behind a progress dot too)
    if not rows:
        sys.exit(f"{log}: no {TAG.strip()} line (run pytest with -s)")
    kinds = {r["test"] for r in rows}
    missing = [k for k in EXPECTED if k not in kinds]
    if missing:
        sys.exit(f"{log}: no row of kind {', '.join(missing)}: not a full run of tests/test_gpu_normal_render.py; nothing written")
    E = {}
    for r in rows:
        if r["test"] in ("forward", "backward"):
            E.setdefault(r["case"], {})[r["test"]] = r["E_kernel"]
    bad = [c for c, d in E.items() if set(d) != {"forward", "backward"}]
    if bad:
        sys.exit(f"{log}: {', '.join(sorted(bad))} without both a forward and a backward row; nothing written")
    os.makedirs(os.path.join(ROOT, "profiles", "normal_render"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "normal_render", "margins.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    path = os.path.join(ROOT, "tests", "golden", "normal_render_margins.json")
    with open(path) as f:
        g = json.load(f)
    g["E_kernel"] = E
    with open(path, "w") as f:
        json.dump(g, f, indent=1, sort_keys=True)
        f.write("\n")
    for case, d in E.items():
        print(f"{case:22s} forward {d['forward']:.3e}  backward " + "  ".join(f"{k} {v:.3e}" for k, v in sorted(d["backward"].items())))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
