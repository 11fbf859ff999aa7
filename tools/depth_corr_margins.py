#!/usr/bin/env python3
"""tools/depth_corr_margins.py OUT.json [--kernels] [--composition] [--trainer]: measure, on an MI355X, what
tests/test_gpu_depth_corr.py holds the Pearson-correlation depth loss to, and write it in the layout of
tests/golden/depth_corr_margins.json (an existing OUT.json keeps the part not measured).
  --kernels      the worst error ratio of loss, gradient and fit over the test's case matrix against the float64 yardstick
                 (tests/depth_corr_reference.py), one line per case to stdout, every exact property asserted; K = 10 x worst.
  --composition  the worst change of the parameter gradients of the test's small scene under target -> 2.5 target + 0.3, the largest
                 of three repetitions (the backward's float atomics are in it); K = 10 x worst.
  --trainer      examples/train.py in hidden-scene mode, 100 x 100, 8 views, 300 iterations, --depth-noise 1, with --depth-loss l1,
                 --depth-loss pearson and --lambda-depth 0, for --depth-seed 0, 1, 2, one run each: the gaps in clean depth L1 between
                 l1 and pearson, and the required gap (half the smallest; none when a gap is not positive: the claim then does not hold)."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import conftest  # noqa: E402
import depth_corr_reference as R  # noqa: E402
import test_gpu_depth_corr as T  # noqa: E402

out_path, what = sys.argv[1], set(sys.argv[2:]) or {"--kernels", "--composition", "--trainer"}
out = json.load(open(out_path)) if os.path.exists(out_path) else {}
if "--kernels" in what:
    worst = T.measure_kernels(T.make_cases())
    for k, w in worst.items():
        out[k] = {"worst": w, "K": 10.0 * w}
if "--composition" in what:
    reps = [T.composition_ratio(conftest.sub("scenes"), conftest.sub("cameras"))[0] for _ in range(3)]
    out["composition"] = {"worst": max(reps), "K": 10.0 * max(reps), "repetitions": reps}
if "--trainer" in what:
    tr = {"command": f"examples/train.py --size 100 --views 8 --iterations 300 --depth-noise 1 --depth-seed S "
                     f"[--lambda-depth {T.LAMBDA_DEPTH} --depth-loss l1|pearson | --lambda-depth 0]", "seeds": [0, 1, 2]}
    keys = {"clean_depth_l1": "train_depth_l1_clean_mean", "depth_l1_as_given": "train_depth_l1_mean", "rho": "train_depth_corr_mean",
            "psnr": "train_psnr_mean", "it_s": "iterations_per_s"}
    runs = {label: {k: [] for k in keys} for label in ("l1", "pearson", "none")}
    with tempfile.TemporaryDirectory() as tmp:
        for seed in tr["seeds"]:
            for label, s in T.trainer_trio(tmp, seed).items():
                for k, field in keys.items():
                    runs[label][k].append(s[field])
                print(label, seed, {k: runs[label][k][-1] for k in keys}, flush=True)
    for label in runs:
        for k in keys:
            tr[f"{label}_{k}"] = runs[label][k]
    tr["gaps"] = [a - b for a, b in zip(tr["l1_clean_depth_l1"], tr["pearson_clean_depth_l1"])]
    tr["claim_holds"] = min(tr["gaps"]) > 0                   # pearson below l1 for every seed; otherwise no gap is required of the test
    tr["required_gap"] = 0.5 * min(tr["gaps"]) if tr["claim_holds"] else None
    out["trainer"] = tr
out["_note"] = ("loss / grad / fit: the largest error of each output on the case matrix of tests/depth_corr_reference.py against the float64 "
                "yardstick, in units of eps32 times the error model (tests/test_gpu_depth_corr.py), measured on an MI355X; K = 10 x worst is "
                "the bound.  composition: the largest change of a parameter gradient under target -> 2.5 target + 0.3, in eps32 of its "
                "largest element, the worst of three repetitions.  trainer: single runs per seed on an MI355X; clean_depth_l1 = the masked "
                "inverse-depth L1 against the unperturbed targets; gaps = l1 - pearson; required_gap = half the smallest, or null with claim_holds false when a gap is not positive")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", out_path)
