#!/usr/bin/env python3
"""Put one MI355X run of tests/test_gpu_blend_grad.py on file.  usage: record_blend_grad_margins.py LOG

LOG is the output of `pytest -s -m gpu tests/test_gpu_blend_grad.py`.  Its BLEND_GRAD_ROW lines (one per case, kernel path, block
shape and gradient array, the child processes' among them) become profiles/blend_grad/margins.jsonl as they are, and the worst
E_spread and E_kernel per case and array, with the E_oracle and the smallest bound they were held to, the "gpu" entry of
tests/golden/blend_grad_margins.json.  Nothing else in that file changes.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "BLEND_GRAD_ROW "


def main(log):
    with open(log) as f:
        rows = [json.loads(l[len(TAG):]) for l in f if l.startswith(TAG)]
    if not rows:
        sys.exit(f"{log}: no {TAG.strip()} line (run pytest with -s)")
    with open(os.path.join(ROOT, "profiles", "blend_grad", "margins.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    gpu = {}
    for r in rows:
        d = gpu.setdefault(r["case"], {}).setdefault(r["array"], {"E_oracle": r["E_oracle"], "E_spread": 0.0, "E_kernel": 0.0, "bound": r["bound"], "rows": 0})
        d["E_spread"], d["E_kernel"] = max(d["E_spread"], r["E_spread"]), max(d["E_kernel"], r["E_kernel"])
        d["bound"] = min(d["bound"], r["bound"])
        d["rows"] += 1
    path = os.path.join(ROOT, "tests", "golden", "blend_grad_margins.json")
    with open(path) as f:
        g = json.load(f)
    g["gpu"] = gpu
    with open(path, "w") as f:
        json.dump(g, f, indent=1, sort_keys=True)
    for case, arrays in gpu.items():
        for k, d in arrays.items():
            print(f"{case:18s} {k:16s} E_oracle {d['E_oracle']:.3e}  E_spread {d['E_spread']:.3e}  E_kernel {d['E_kernel']:.3e}  "
                  f"smallest bound {d['bound']:.3e}  ({d['rows']} rows)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
