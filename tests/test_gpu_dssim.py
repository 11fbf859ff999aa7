"""The L1 + D-SSIM kernels (include/gsr_loss.h) on the MI355X, against the float64 definition of tests/dssim_reference.py:
L1 sum, SSIM sum and pixel_grad for both windows and lambda in {0.2, 1}, at the sizes of test_dssim_reference.py, 800 x 800, odd
sizes, images smaller than the window, constant images and a rendered image slightly outside [0, 1].  Then the contracts:
gsr_ssim's sum with the reference window, gsr_l1_loss_grad's gradient bit for bit at lambda = 0, a vanishing SSIM gradient at
rendered == target, bit-identical repeat calls, untouched canary words, and a short trainer run with --lambda-dssim 0.2.

Tripwires (measured margins in profiles/dssim_kernels/margins.jsonl): about 10x the largest margin measured.  Constant images are
held apart: with zero variance D = C2, and float32 cancellation in e11 - m1^2 (the reference's ssim_kernel has the same) sets
their margins (max|dg| 2.1e-4 max|g|, SSIM 2.9e-5); their gradient bound is the 1e-3 max|g_f64| ceiling, under 10x."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dssim_reference as R
from conftest import ROOT, sub

pytestmark = pytest.mark.gpu

GRAD_TOL = 6e-5        # max|dg| / max|g_f64|                      (largest margin measured 5.9e-6)
SSIM_TOL = 1.3e-5      # |dssim_sum| / (H W), i.e. on the mean SSIM (1.3e-6)
L1_TOL = 1e-6          # relative                                  (1.0e-7)
TOL_CONSTANT = {"grad": 1e-3, "ssim": 3e-4, "l1": 1e-6}

SIZES = [(1, 1), (5, 9), (16, 16), (17, 33), (64, 48), (200, 300), (800, 800), (31, 17), (33, 15), (97, 61), (3, 4), (10, 10)]


def images(W, H, kind="noisy", seed=0):
    rng = np.random.default_rng(seed + 7919 * W + H)
    t = rng.random((H, W, 3), dtype=np.float32)
    if kind == "noisy":
        r = np.clip(t + rng.normal(0, 0.1, t.shape).astype(np.float32), 0, 1)
    elif kind == "outside":                                  # a rendered image a little outside [0, 1]
        r = (t + rng.normal(0, 0.1, t.shape).astype(np.float32)) * np.float32(1.1) - np.float32(0.05)
    elif kind == "constant":
        r, t = np.full_like(t, 0.3), np.full_like(t, 0.7)
    return r.astype(np.float32), t


def gpu(a):
    return torch.as_tensor(a).cuda()


def run(r, t, lam, window, want_grad=True):
    loss = sub("loss")
    l1, ss, g = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(t), lam, window=window, want_grad=want_grad)
    torch.cuda.synchronize()
    return float(l1.item()), float(ss.item()), (g.cpu().double() if g is not None else None)


def margins(r, t, lam, window):
    W, H = r.shape[1], r.shape[0]
    l1, ss, g = run(r, t, lam, window)
    x, y = torch.as_tensor(r, dtype=R.F64).cuda(), torch.as_tensor(t, dtype=R.F64).cuda()
    gr = R.pixel_grad(x, y, lam, window).cpu()
    l1r, ssr = float(R.l1_sum(x, y)), float(R.ssim_sum(x, y, window))
    return {"grad": float((g - gr).abs().max() / gr.abs().max()), "ssim": abs(ss - ssr) / (W * H),
            "l1": abs(l1 - l1r) / max(l1r, 1e-30)}


CASES = [(W, H, "noisy") for W, H in SIZES] + [(64, 48, "outside"), (800, 800, "outside"), (17, 33, "constant"), (4, 3, "constant")]


@pytest.mark.parametrize("W,H,kind", CASES)
@pytest.mark.parametrize("window", ["gaussian", "reference"])
@pytest.mark.parametrize("lam", [0.2, 1.0])
def test_against_the_float64_definition(W, H, kind, window, lam):
    m = margins(*images(W, H, kind), lam, window)
    print(json.dumps({"W": W, "H": H, "kind": kind, "window": window, "lambda": lam, **m}))
    tol = TOL_CONSTANT if kind == "constant" else {"grad": GRAD_TOL, "ssim": SSIM_TOL, "l1": L1_TOL}
    assert all(m[k] <= tol[k] for k in tol), m


@pytest.mark.parametrize("W,H", [(16, 16), (200, 300), (800, 800), (33, 15)])
def test_reference_window_is_gsr_ssim(W, H):
    r, t = images(W, H)
    _, ss, _ = run(r, t, 0.2, "reference", want_grad=False)
    want = sub("loss").ssim(gpu(r), gpu(t))
    assert abs(ss / (W * H) - want) <= 2e-5 * abs(want), (ss / (W * H), want)
    assert sub("loss").ssim(gpu(r), gpu(t), window="gaussian") == run(r, t, 0.0, "gaussian", False)[1] / (W * H)


@pytest.mark.parametrize("W,H", [(800, 800), (17, 33), (1, 1)])
@pytest.mark.parametrize("window", ["gaussian", "reference"])
def test_lambda_zero_is_the_l1_gradient_bit_for_bit(W, H, window):
    r, t = images(W, H)
    t[0, 0] = r[0, 0]                                        # sign(0) = +1 on both paths
    _, want = sub("loss").l1_loss_and_gradients(gpu(r), gpu(t), 0.0)
    l1, _, got = sub("loss").l1_dssim_loss_and_gradients(gpu(r), gpu(t), 0.0, window=window)
    assert torch.equal(got, want)
    assert float(l1.item()) == pytest.approx(float(np.abs(r.astype(np.float64) - t).sum()), rel=L1_TOL)


@pytest.mark.parametrize("W,H", [(800, 800), (37, 21)])
@pytest.mark.parametrize("window", ["gaussian", "reference"])
def test_ssim_gradient_vanishes_at_rendered_equal_target(W, H, window):
    r, t = images(W, H)
    _, ss, g_same = run(t, t, 1.0, window)
    _, _, g_diff = run(r, t, 1.0, window)
    assert ss / (W * H) == pytest.approx(1.0, abs=1e-5)
    assert float(g_same.abs().max()) <= 1e-3 * float(g_diff.abs().max()), (float(g_same.abs().max()), float(g_diff.abs().max()))


@pytest.mark.parametrize("W,H", [(800, 800), (97, 61)])
def test_two_calls_give_the_same_bits(W, H):
    r, t = images(W, H)
    loss = sub("loss")
    a = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(t), 0.2)
    b = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(t), 0.2)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("W,H", [(800, 800), (33, 15), (5, 9)])
def test_canaries_after_pixel_grad_and_workspace(W, H):
    _lib, host = sub("_lib"), sub("_host")
    L = _lib.lib()
    r, t = images(W, H)
    rd, td = gpu(r), gpu(t)
    n, need, pad = H * W * 3, int(L.gsr_dssim_workspace_bytes(W, H)), 4096
    gbuf = torch.full((n + pad,), 1234.5, device="cuda")
    wbuf = torch.full((need // 4 + pad,), -77.25, device="cuda")
    sums = torch.zeros(8, device="cuda")
    rc = L.gsr_l1_dssim_loss_grad(host.ptr(rd), host.ptr(td), host.ptr(gbuf), host.ptr(sums), host.ptr(sums[4:]), W, H, 0.2, 1,
                                  host.ptr(wbuf), need, host.stream_ptr(rd.device))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((gbuf[n:] == 1234.5).all()) and bool((wbuf[need // 4:] == -77.25).all())
    assert bool((sums[1:4] == 0).all()) and bool((sums[5:] == 0).all())
    assert bool(torch.isfinite(gbuf[:n]).all())


def test_short_training_run_with_dssim(tmp_path):
    log = tmp_path / "train.jsonl"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train.py"), "--dataset", os.path.join(ROOT, "data", "lego"), "--views", "8",
           "--iterations", "300", "--gaussians", "5000", "--lambda-dssim", "0.2", "--print-interval", "50", "--log", str(log)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    recs = [json.loads(l) for l in open(log)]
    summary = [r for r in recs if r["record"] == "summary"][0]
    l1 = np.concatenate([np.asarray(r["l1"], np.float64) for r in recs if r["record"] == "loss"])
    ss = np.concatenate([np.asarray(r["ssim"], np.float64) for r in recs if r["record"] == "loss"])
    combined = 0.8 * l1 + 0.2 * (1.0 - ss)
    print(f"\ncombined loss first/last 20: {combined[:20].mean():.5f} / {combined[-20:].mean():.5f}; SSIM {ss[0]:.4f} -> {ss[-20:].mean():.4f}; "
          f"train SSIM {summary['train_ssim_mean']:.4f}, PSNR {summary['train_psnr_mean']:.2f} dB, {summary['iterations_per_s']} it/s")
    assert len(l1) == len(ss) == 300 and np.isfinite(combined).all()
    assert all(summary["parameters_finite"].values())
    assert combined[-20:].mean() < 0.85 * combined[:20].mean()
    assert ss[-20:].mean() > ss[0] and summary["train_ssim_mean"] > ss[0]
    printed = [float(l.split()[-1]) for l in p.stdout.splitlines() if l.startswith("iter") and "loss" in l and "densify" not in l]
    assert printed and abs(printed[0] - combined[0]) <= 1e-4, (printed[0], combined[0])
