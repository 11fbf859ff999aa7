#!/usr/bin/env python3
"""Put one MI355X run of tests/test_gpu_median_depth.py on file.  usage: record_median_depth_margins.py LOG

LOG is the output of `pytest -s -m gpu tests/test_gpu_median_depth.py`.  Its MEDIAN_DEPTH_ROW lines become
profiles/median_depth/margins.jsonl as they are, and per frame the E_kernel of the backward -- measured against the float64
scatter-add, never against the kernel itself -- the "E_backward" entry of tests/golden/median_depth_margins.json: from then on the
test also fails above 10 x that value.  "tie_share" (CPU, tests/test_median_depth_reference.py prints it) and "mesh_gap_min" are left
as they are.  A log without a row of every kind the tests print, or without a backward row for every frame of the matrix, is refused
and nothing is written."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "MEDIAN_DEPTH_ROW "
EXPECTED = ("forward", "backward", "backward_view", "torus", "trainer")


def main(log):
    with open(log) as f:
        rows = [json.loads(l[l.index(TAG) + len(TAG):]) for l in f if TAG in l]      # (anywhere in a line: behind a progress dot too)
    if not rows:
        sys.exit(f"{log}: no {TAG.strip()} line (run pytest with -s)")
    kinds = {r["test"] for r in rows}
    missing = [k for k in EXPECTED if k not in kinds]
    if missing:
        sys.exit(f"{log}: no row of kind {', '.join(missing)}: not a full run of tests/test_gpu_median_depth.py; nothing written")
    path = os.path.join(ROOT, "tests", "golden", "median_depth_margins.json")
    with open(path) as f:
        g = json.load(f)
    E = {}
    for r in rows:
        if r["test"] == "backward":
            E[r["case"]] = max(E.get(r["case"], 0.0), r["E_kernel"])
    if set(E) != set(g["tie_share"]):
        sys.exit(f"{log}: backward rows for {sorted(E)}, the matrix has {sorted(g['tie_share'])}; nothing written")
    os.makedirs(os.path.join(ROOT, "profiles", "median_depth"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "median_depth", "margins.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    g["E_backward"] = E
    with open(path, "w") as f:
        json.dump(g, f, indent=1, sort_keys=True)
        f.write("\n")
    for case, v in E.items():
        print(f"{case:22s} backward {v:.3e}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
