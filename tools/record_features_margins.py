#!/usr/bin/env python3
"""Put one MI355X run of tests/test_gpu_features.py on file.  usage: record_features_margins.py LOG

LOG is the output of `pytest -s -m gpu tests/test_gpu_features.py`.  Its FEATURES_ROW lines become profiles/features/margins.jsonl as
they are, and per frame the worst E_kernel of the forward and of the backward over the channel counts, and the largest difference
from the product's own image, 1 - final_Ts and inverse-depth image, the "E_kernel" entry of tests/golden/features_margins.json: from
then on the tests also fail above 3 x those values.  "floor" (the smallest float32-restatement error of the CPU matrix,
tests/test_features_reference.py prints it) is left as it is.  A log without a row of every kind the tests print, or without every
frame's rows for every channel count, is refused and nothing is written.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "FEATURES_ROW "
EXPECTED = ("forward", "forward_worst", "own_images", "backward", "backward_worst", "dL_dcolor", "one_hot", "autograd", "fit_features")
CHANNELS = (1, 3, 4, 5, 16, 17, 64)      # tests/test_gpu_features.py: a forward row per frame and C, a backward row per frame, C and path


def main(log):
    with open(log) as f:
        rows = [json.loads(l[l.index(TAG) + len(TAG):]) for l in f if TAG in l]      # (anywhere in a line: behind a progress dot too)
    if not rows:
        sys.exit(f"{log}: no {TAG.strip()} line (run pytest with -s)")
    kinds = {}
    for r in rows:
        kinds[r["test"]] = kinds.get(r["test"], 0) + 1
    missing = [k for k in EXPECTED if k not in kinds]
    if missing:
        sys.exit(f"{log}: no row of kind {', '.join(missing)}: not a full run of tests/test_gpu_features.py; nothing written")
    frames = {r["case"] for r in rows if r["test"] == "forward_worst"}
    for kind, per_frame in (("forward", len(CHANNELS)), ("backward", 2 * len(CHANNELS)), ("own_images", 1)):
        for case in sorted(frames):
            n = sum(1 for r in rows if r["test"] == kind and r["case"] == case)
            if n != per_frame:
                sys.exit(f"{log}: {n} '{kind}' rows for {case}, expected {per_frame}; nothing written")
    os.makedirs(os.path.join(ROOT, "profiles", "features"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "features", "margins.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    E = {}
    for r in rows:
        if r["test"] in ("forward", "backward"):
            d = E.setdefault(r["case"], {})
            d[r["test"]] = max(d.get(r["test"], 0.0), r["E_kernel"])
        elif r["test"] == "own_images":
            d = E.setdefault(r["case"], {})
            for k in ("image", "alpha", "inv_depth"):
                d["own_" + k] = max(d.get("own_" + k, 0.0), r[k])
    path = os.path.join(ROOT, "tests", "golden", "features_margins.json")
    with open(path) as f:
        g = json.load(f)
    g["E_kernel"] = E
    with open(path, "w") as f:
        json.dump(g, f, indent=1, sort_keys=True)
    for case, d in E.items():
        print(f"{case:22s} " + "  ".join(f"{k} {v:.3e}" for k, v in sorted(d.items())))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
