"""examples/train.py with its flags TOGETHER: every other trainer test switches on one feature, and what breaks when the step's state
moves is a combination.  Three small hidden-scene runs (64 x 64, 4 views, 2 000 Gaussians, 30 iterations, density control at 10, 15
and an opacity reset every 7): A with everything one GPU allows, B in capacity mode with three views on three streams, C through the
other branches (dense SH gradient, two views in turn, the Pearson depth loss on perturbed targets, noisy normals, poses and exposures).
The assertions are about structure -- the run ends, stays finite, and writes every record, key and file its flags promise; the bounds
on what is learnt belong to each feature's own test."""
import json
import math
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

COMMON = ["--size", "64", "--views", "4", "--gaussians", "2000", "--iterations", "30", "--densify-from", "5", "--densify-interval", "5",
          "--densify-until", "20", "--opacity-reset-interval", "7", "--print-interval", "1000"]


def _train(tmp, *extra):
    """(records, summary) of one run; the checks every run shares."""
    log = os.path.join(tmp, "run.jsonl")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), *COMMON, "--log", log, *extra],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    records = [json.loads(ln) for ln in open(log)]
    assert records[0]["record"] == "arguments" and "init" in records[0] and "first_iteration_pairs" in records[0]
    summary = records[-1]
    assert summary["record"] == "summary" and all(summary["parameters_finite"].values()) and len(summary["parameters_finite"]) == 5
    return records, summary


def _curve(records, key):
    out = [x for r in records if r["record"] == "loss" and key in r for x in r[key]]
    assert all(isinstance(x, float) and math.isfinite(x) for x in out), out
    return out


def test_everything_one_gpu_allows(tmp_path):
    out, evald, mesh = tmp_path / "out", tmp_path / "eval", tmp_path / "mesh.ply"
    records, s = _train(str(tmp_path), "--lambda-dssim", "0.2", "--lambda-depth", "0.5", "--lambda-alpha", "0.1", "--lambda-normal", "0.05",
                        "--optimize-exposure", "--optimize-poses", "--filter-3d", "--filter-3d-interval", "2", "--rasterize-mode", "antialiased",
                        "--densify-stat", "screen", "--absgrad", "--occluders", "1", "--mask-occluders", "--init", "knn", "--eval-scales", "1,2",
                        "--output", str(out), "--save-interval", "10", "--eval-dir", str(evald), "--mesh-out", str(mesh), "--mesh-resolution", "32")
    assert len(_curve(records, "l1")) == 30 and len(_curve(records, "ssim")) == 30
    for key in ("train_weighted_l1_mean", "train_weighted_psnr_mean", "train_weighted_ssim_mean", "clean_psnr_mean", "pose_error_start",
                "pose_error_final", "exposure_final", "exposure_steps", "train_depth_l1_mean", "train_depth_corr_mean", "train_alpha_l1_mean",
                "train_normal_angle_deg_mean", "train_eval_scales"):
        assert key in s, key
    assert set(s["train_eval_scales"]) == {"1", "2"}
    filters = [r for r in records if r["record"] == "filter_3d"]
    assert filters[0]["why"] == "start" and len(filters) >= 2
    last = out / "point_cloud" / "iteration_29"
    assert (last / "point_cloud.ply").stat().st_size > 0 and json.load(open(last / "exposure.json"))
    assert (evald / "render_0.png").stat().st_size > 0
    assert mesh.stat().st_size > 0


def test_capacity_mode_with_views_on_streams(tmp_path):
    records, s = _train(str(tmp_path), "--capacity", "--views-per-step", "3", "--view-streams", "3", "--lambda-dssim", "0.2",
                        "--ssim-window", "reference", "--densify-stat", "screen")
    assert len(_curve(records, "l1")) == 30 and len(_curve(records, "ssim")) == 30
    retries = [r for r in records if r["record"] == "capacity_retry"]
    assert s["capacity_retries"] == len(retries)
    for r in retries:
        assert r["D"] > r["capacity"], r


def test_the_other_branches(tmp_path):
    records, s = _train(str(tmp_path), "--dense-sh", "--views-per-step", "2", "--depth-loss", "pearson", "--lambda-depth", "1", "--depth-noise", "1",
                        "--lambda-normal", "0.05", "--normal-noise", "0.1", "--init", "random", "--pose-noise-deg", "1", "--pose-noise-trans", "0.02",
                        "--exposure-noise", "0.2")
    assert len(_curve(records, "l1")) == 30
    for key in ("train_depth_l1_clean_mean", "pose_error_start", "pose_error_final"):
        assert key in s, key
