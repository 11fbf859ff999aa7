"""CPU checks that pin the float64 D-SSIM definition (tests/dssim_reference.py) before any kernel is held to it: with the
reference window it is the oracle's SSIM (which restates the reference's ssim_kernel), autograd agrees with the closed-form
alpha / beta / gamma maps of include/gsr_loss.h and with central differences, and a wrong window or border rule is caught."""
import math

import numpy as np
import pytest
import torch

import dssim_reference as R

SIZES = [(1, 1), (5, 9), (16, 16), (17, 33), (64, 48), (200, 300)]   # (W, H)


def pair(W, H, seed=0):
    rng = np.random.default_rng(seed + 1000 * W + H)
    r = rng.random((H, W, 3), dtype=np.float32)
    t = np.clip(r + rng.normal(0, 0.1, (H, W, 3)).astype(np.float32), 0, 1)
    return r, t


def f32_sum_tol(n):
    """float32 error of the oracle's serial sum of n per-pixel values near 1, on the mean: a few ulp(n) random-walked over n adds"""
    return 1e-6 + 4.0 * 2.0 ** (math.floor(math.log2(n)) - 24) / math.sqrt(n)


@pytest.mark.parametrize("W,H", SIZES)
def test_reference_window_is_the_oracle_ssim(oracle, W, H):
    r, t = pair(W, H)
    got = float(R.ssim_sum(torch.as_tensor(r, dtype=R.F64), torch.as_tensor(t, dtype=R.F64), "reference")) / (W * H)
    assert abs(got - oracle.ssim(r, t)) <= f32_sum_tol(W * H), (got, oracle.ssim(r, t))


@pytest.mark.parametrize("W,H", [(5, 9), (16, 16), (17, 33), (64, 48)])
@pytest.mark.parametrize("window", ["reference", "gaussian"])
def test_autograd_is_the_closed_form(W, H, window):
    r, t = pair(W, H, 1)
    x, y = torch.as_tensor(r, dtype=R.F64), torch.as_tensor(t, dtype=R.F64)
    g = R.pixel_grad(x, y, 1.0, window)                  # lambda = 1: -dSSIM/dx alone
    c = R.closed_form_grad(x, y, window)
    assert torch.allclose(-g, c, rtol=1e-9, atol=1e-12 * float(c.abs().max()))


@pytest.mark.parametrize("window", ["reference", "gaussian"])
@pytest.mark.parametrize("lam", [0.2, 1.0])
def test_gradient_matches_central_differences(window, lam):
    W, H = 13, 7
    r, t = pair(W, H, 2)
    x, y = torch.as_tensor(r, dtype=R.F64), torch.as_tensor(t, dtype=R.F64)
    g = R.pixel_grad(x, y, lam, window)
    h = 1e-6
    rng = np.random.default_rng(3)
    for _ in range(25):
        j, i, c = int(rng.integers(H)), int(rng.integers(W)), int(rng.integers(3))
        xp, xm = x.clone(), x.clone()
        xp[j, i, c] += h
        xm[j, i, c] -= h
        fd = float(R.loss(xp, y, lam, window) - R.loss(xm, y, lam, window)) / (2 * h)
        assert abs(fd - float(g[j, i, c])) <= 1e-7 * float(g.abs().max()), (j, i, c, fd, float(g[j, i, c]))


def test_power_a_wrong_window_or_border_rule_fails_the_oracle(oracle):
    for W, H in [(16, 16), (64, 48)]:
        r, t = pair(W, H)
        x, y = torch.as_tensor(r, dtype=R.F64), torch.as_tensor(t, dtype=R.F64)
        want, tol = oracle.ssim(r, t), f32_sum_tol(W * H)
        swapped = float(R.ssim_sum(x, y, "gaussian")) / (W * H)
        padded = float(R.ssim_sum(x, y, "reference", renorm=False)) / (W * H)
        assert abs(swapped - want) > 10 * tol and abs(padded - want) > 10 * tol, (want, swapped, padded, tol)
