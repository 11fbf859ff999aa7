#!/usr/bin/env python3
"""Put one run of the plane-depth tests on file.  usage: record_plane_depth_margins.py LOG

LOG is the output of `pytest -s tests/test_plane_depth_reference.py` (CPU) or of `pytest -s -m gpu tests/test_gpu_plane_depth.py`
(MI355X).  The PLANE_DEPTH_F32 lines of a CPU log become "E_f32" and "floor" (the smallest of the frames' worst errors) of
tests/golden/plane_depth_margins.json: the float32 restatement's errors against the float64 yardstick, which the GPU test's bounds are
made of.  The PLANE_DEPTH_ROW lines of a GPU log become profiles/plane_depth/margins.jsonl as they are, and the E_kernel of every
frame's backward row the "E_kernel" entry of the JSON -- a record only: no test reads it as a bound.  "mesh_gap_min" stays null.  A log
with neither kind of line is refused and nothing is written."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, ROW = "PLANE_DEPTH_F32 ", "PLANE_DEPTH_ROW "
PATH = os.path.join(ROOT, "tests", "golden", "plane_depth_margins.json")


def rows_of(log, tag):
    with open(log) as f:
        # (anywhere in a line: behind a progress dot too; a traceback's source line that names the tag carries no row)
        return [json.loads(l[l.index(tag) + len(tag):]) for l in f if tag + "{" in l and l.rstrip().endswith("}")]


def main(log):
    cpu, gpu = rows_of(log, F32), rows_of(log, ROW)
    if not cpu and not gpu:
        sys.exit(f"{log}: neither a {F32.strip()} nor a {ROW.strip()} line (run pytest with -s)")
    g = {"E_f32": {}, "E_kernel": {}, "floor": 0.0, "mesh_gap_min": None}
    if os.path.exists(PATH):
        with open(PATH) as f:
            g = json.load(f)
    if cpu:
        g["E_f32"] = {r["case"]: r["E_f32"] for r in cpu}
        g["floor"] = min(max(e.values()) for e in g["E_f32"].values())
    if gpu:
        g["E_kernel"] = {r["case"]: r["E_kernel"] for r in gpu if r["test"] == "backward"}
        os.makedirs(os.path.join(ROOT, "profiles", "plane_depth"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "plane_depth", "margins.jsonl"), "w") as f:
            for r in gpu:
                f.write(json.dumps(r) + "\n")
    with open(PATH, "w") as f:
        json.dump(g, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(g, indent=1, sort_keys=True))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
