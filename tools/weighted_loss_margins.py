#!/usr/bin/env python3
"""tools/weighted_loss_margins.py OUT.json [--kernels] [--trainer]: measure, on an MI355X, what tests/test_gpu_weighted_loss.py holds
the weighted colour loss to, and write it in the layout of tests/golden/weighted_loss_margins.json (an existing OUT.json keeps the
part not measured).
  --kernels  the largest error of every case of the test's own list against the float64 definition ("kernels"), one line per case
             to stdout; the all-zero cases must give exact zeros.
  --trainer  examples/train.py on the eight Lego views, 300 iterations, --lambda-dssim 0.2 --occluders 3, with and without
             --mask-occluders, for --occluder-seed 0, 1, 2, one run each ("trainer"): the gaps in clean PSNR and clean L1, the
             required gaps (half the smallest) and the plain run's spread over the seeds."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_weighted_loss as T  # noqa: E402

out_path, what = sys.argv[1], set(sys.argv[2:]) or {"--kernels", "--trainer"}
out = json.load(open(out_path)) if os.path.exists(out_path) else {}
if "--kernels" in what:
    worst = {"grad": 0.0, "ssim": 0.0, "l1": 0.0, "total": 0.0}
    for W, H, kind in T.CASES:
        for window in T.WINDOWS:
            for lam in T.LAMBDAS:
                m = T.case_margins(W, H, kind, window, lam)
                print(json.dumps({"W": W, "H": H, "kind": kind, "window": window, "lambda": lam, **m}), flush=True)
                if m["zero"]:
                    assert m["grad"] == m["ssim"] == m["l1"] == m["total"] == 0.0, m
                else:
                    worst = {k: max(worst[k], m[k]) for k in worst}
    out["kernels"] = dict(worst, cases=len(T.CASES) * len(T.WINDOWS) * len(T.LAMBDAS))
if "--trainer" in what:
    tr = {"command": "examples/train.py --dataset data/lego --views 8 --iterations 300 --lambda-dssim 0.2 --occluders 3 --occluder-seed S [--mask-occluders]",
          "seeds": [0, 1, 2]}
    keys = ("clean_psnr", "clean_l1", "clean_ssim", "it_s")
    runs = {"plain": {k: [] for k in keys}, "masked": {k: [] for k in keys}}
    with tempfile.TemporaryDirectory() as tmp:
        for seed in tr["seeds"]:
            for label, extra in (("plain", ()), ("masked", ("--mask-occluders",))):
                s = T.trainer_run(tmp, f"{label}{seed}", "--occluders", "3", "--occluder-seed", str(seed), *extra)
                for k, v in zip(keys, (s["clean_psnr_mean"], s["clean_l1_mean"], s["clean_ssim_mean"], s["iterations_per_s"])):
                    runs[label][k].append(v)
                print(label, seed, {k: runs[label][k][-1] for k in keys}, flush=True)
    for label in runs:
        for k in keys:
            tr[f"{label}_{k}"] = runs[label][k]
    tr["psnr_gaps"] = [a - b for a, b in zip(tr["masked_clean_psnr"], tr["plain_clean_psnr"])]
    tr["l1_gaps"] = [b - a for a, b in zip(tr["masked_clean_l1"], tr["plain_clean_l1"])]
    tr["required_psnr_gap"], tr["required_l1_gap"] = 0.5 * min(tr["psnr_gaps"]), 0.5 * min(tr["l1_gaps"])
    tr["plain_psnr_spread"] = max(tr["plain_clean_psnr"]) - min(tr["plain_clean_psnr"])
    tr["plain_l1_spread"] = max(tr["plain_clean_l1"]) - min(tr["plain_clean_l1"])
    out["trainer"] = tr
out["_note"] = ("kernels: the largest error over the case list of tests/test_gpu_weighted_loss.py against the float64 definition "
                "(tests/weighted_loss_reference.py), measured once on one MI355X: max|dg| / max|g_f64|, |dssim_sum| / M, relative for the L1 sum "
                "and M; the tripwires are 10 x these, the gradient's at most 1e-3.  trainer: single runs per seed on one MI355X, scored against "
                "the clean targets; required gaps = half the smallest measured gap; spreads = max - min of the plain run over the seeds")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", out_path)
