"""CPU checks that pin the float64 statement of the weighted colour loss (tests/weighted_loss_reference.py) before any kernel is held
to it: the closed form is autograd's gradient, all-ones weights give dssim_reference's loss, k m is m, nothing outside the weights'
5-pixel reach receives a gradient while a weight-0 pixel inside it does, M = 0 gives zeros, and under weights that are 0 on a
region grown by the window radius the region's content is invisible, bit for bit."""
import numpy as np
import pytest
import torch

import dssim_reference as R
import weighted_loss_reference as WR

F64 = R.F64


def pair(W, H, seed=0):
    rng = np.random.default_rng(seed + 1000 * W + H)
    t = rng.random((H, W, 3))
    r = np.clip(t + rng.normal(0, 0.1, (H, W, 3)), 0, 1)
    return torch.as_tensor(r, dtype=F64), torch.as_tensor(t, dtype=F64)


def smooth_weights(W, H, seed=0):
    """floats in [0, 2] that vary over a few pixels"""
    rng = np.random.default_rng(seed + 31 * W + H)
    yy, xx = np.mgrid[0:H, 0:W]
    a, b, p = rng.uniform(0.1, 0.5, 2), rng.uniform(0.1, 0.5, 2), rng.uniform(0, 6.28, 2)
    return torch.as_tensor(1.0 + np.sin(a[0] * xx + b[0] * yy + p[0]) * np.cos(a[1] * xx - b[1] * yy + p[1]), dtype=F64)


def hole_weights(W, H):
    """ones with a rectangular hole of zeros"""
    m = torch.ones((H, W), dtype=F64)
    m[H // 4:H // 4 + max(1, H // 3), W // 3:W // 3 + max(1, W // 4)] = 0.0
    return m


@pytest.mark.parametrize("W,H", [(5, 9), (17, 33), (40, 24)])
@pytest.mark.parametrize("window", ["reference", "gaussian"])
@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
def test_closed_form_is_autograd(W, H, window, lam):
    x, y = pair(W, H, 1)
    for m in (smooth_weights(W, H), hole_weights(W, H)):
        c, a = WR.pixel_grad(x, y, m, lam, window), WR.autograd_grad(x, y, m, lam, window)
        assert float((c - a).abs().max()) <= 1e-12 * float(a.abs().max())


@pytest.mark.parametrize("W,H", [(1, 1), (5, 9), (17, 33), (64, 48)])
@pytest.mark.parametrize("window", ["reference", "gaussian"])
def test_all_ones_is_the_unweighted_loss(W, H, window):
    x, y = pair(W, H, 2)
    m = torch.ones((H, W), dtype=F64)
    for lam in (0.0, 0.2, 1.0):
        assert float(WR.loss(x, y, m, lam, window)) == pytest.approx(float(R.loss(x, y, lam, window)), rel=1e-13)
        g, want = WR.pixel_grad(x, y, m, lam, window), R.pixel_grad(x, y, lam, window)
        assert float((g - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float(WR.l1_sum(x, y, m)) == pytest.approx(float(R.l1_sum(x, y)), rel=1e-14)
    assert float(WR.ssim_sum(x, y, m, window)) == pytest.approx(float(R.ssim_sum(x, y, window)), rel=1e-13)


@pytest.mark.parametrize("k", [4.0, 0.3, 1e3])
def test_scaling_the_weights_changes_nothing(k):
    W, H = 33, 21
    x, y = pair(W, H, 3)
    m = smooth_weights(W, H)
    assert float(WR.loss(x, y, k * m, 0.2)) == pytest.approx(float(WR.loss(x, y, m, 0.2)), rel=1e-13)
    g, gk = WR.pixel_grad(x, y, m, 0.2), WR.pixel_grad(x, y, k * m, 0.2)
    assert float((g - gk).abs().max()) <= 1e-13 * float(g.abs().max())
    assert float(WR.l1_sum(x, y, k * m)) == pytest.approx(k * float(WR.l1_sum(x, y, m)), rel=1e-14)


@pytest.mark.parametrize("window", ["reference", "gaussian"])
def test_the_gradient_lives_within_the_window_radius_of_the_weights(window):
    W, H = 48, 40
    x, y = pair(W, H, 4)
    m = torch.zeros((H, W), dtype=F64)
    m[10:14, 20:23] = 1.5
    g = WR.pixel_grad(x, y, m, 0.2, window)
    reach = WR.reach(m)
    assert int(reach.sum()) == (4 + 10) * (3 + 10)
    assert bool((g[~reach] == 0).all())                                   # exactly zero: every term carries a zero weight
    ring = reach & ~(m > 0)
    assert float(g[ring].abs().min()) > 0.0                               # weight 0, but inside a weighted pixel's window
    assert bool((WR.pixel_grad(x, y, m, 0.0, window)[ring] == 0).all())   # ... an SSIM effect: the L1 term stays on the weights


def test_zero_total_gives_zeros():
    x, y = pair(9, 7, 5)
    m = torch.zeros((7, 9), dtype=F64)
    assert float(WR.l1_sum(x, y, m)) == 0.0 and float(WR.ssim_sum(x, y, m)) == 0.0
    assert bool((WR.pixel_grad(x, y, m, 0.2) == 0).all())


def test_dilate_zeros_grows_the_zero_region_and_clips_at_the_border():
    m = torch.ones((12, 15), dtype=F64)
    m[0, 0] = m[6, 7] = 0.0
    d = WR.dilate_zeros(m, 2)
    want = torch.ones_like(m)
    want[0:3, 0:3] = 0.0
    want[4:9, 5:10] = 0.0
    assert torch.equal(d, want) and WR.dilate_zeros(m, 0) is m
    assert torch.equal(WR.dilate_zeros(torch.ones((3, 4), dtype=F64), 5), torch.ones((3, 4), dtype=F64))   # outside the image is not zero


@pytest.mark.parametrize("window", ["reference", "gaussian"])
@pytest.mark.parametrize("lam", [0.2, 1.0])
def test_a_region_masked_with_a_grown_mask_is_invisible(window, lam):
    """Weights 0 on an occluder and within 5 pixels of it: the three outputs are those of the clean target, bit for bit.  With the
    mask of the occluder alone (not grown) they are not."""
    W, H = 56, 44
    x, y = pair(W, H, 6)
    occluded = y.clone()
    occluded[12:25, 30:41] = torch.tensor([1.0, 0.0, 1.0], dtype=F64)
    tight = torch.ones((H, W), dtype=F64)
    tight[12:25, 30:41] = 0.0
    m = WR.dilate_zeros(tight, WR.RAD) * smooth_weights(W, H)
    for out in (lambda t, w: WR.l1_sum(x, t, w), lambda t, w: WR.ssim_sum(x, t, w, window), lambda t, w: WR.pixel_grad(x, t, w, lam, window)):
        assert torch.equal(out(occluded, m), out(y, m))
    assert not torch.equal(WR.pixel_grad(x, occluded, tight, lam, window), WR.pixel_grad(x, y, tight, lam, window))
    assert not torch.equal(WR.ssim_sum(x, occluded, tight, window), WR.ssim_sum(x, y, tight, window))
