"""The order of the additions behind the image losses' sums, held to the bit on the MI355X: the weight total, the weighted L1 sum,
the three plain sums of the exposure gradient and the L1 sum of both D-SSIM entry points against the numpy model of
tests/fixed_order_sum.py, which adds what the kernels add in their order ("The fixed-order sum").  The inputs (fixed_order_sum.flat_inputs /
tile_inputs) span six decades and cancel by halves; tests/test_fixed_order_sum.py checks that on them the model differs from a
sequential sum and from np.sum, so a changed order fails here.  Sizes: fixed_order_sum.flat_sizes / tile_sizes and exposure_reference.case_sizes."""
import numpy as np
import pytest
import torch

import fixed_order_sum as FS
from conftest import sub
from exposure_reference import case_sizes

pytestmark = pytest.mark.gpu

_lib = sub("_lib")
EXPOSURE = (_lib.EXPOSURE_BLOCK_PIXELS, _lib.EXPOSURE_MAX_BLOCKS)
FLAT_SIZES = FS.flat_sizes()
EXPOSURE_SIZES = FLAT_SIZES + [s for s in case_sizes(*EXPOSURE) if s not in FLAT_SIZES]


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def same_bits(got, want, what):
    got, want = np.asarray(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, FS.F32).reshape(-1), np.asarray(want, FS.F32).reshape(-1)
    print(what, "kernel", got.tolist(), "model", want.tolist())
    assert np.array_equal(FS.bits(got), FS.bits(want)), (what, got.tolist(), want.tolist())


@pytest.mark.parametrize("W,H", FLAT_SIZES)
def test_weight_total_and_weighted_l1_sum(W, H):
    loss = sub("loss")
    q = FS.flat_inputs(W, H, *EXPOSURE)
    m, r, t = q["m"], q["r"], q["t"]
    pw = loss.PixelWeights(gpu(m))
    same_bits(pw.total, FS.weight_total(m), f"weight_total {W}x{H}")
    for want_grad in (True, False):
        s, _ = loss.l1_loss_and_gradients(gpu(r), gpu(t), 0.2, want_grad=want_grad, weights=pw)
        same_bits(s, FS.weighted_l1_sum(r, t, m), f"weighted_l1 loss_sum {W}x{H} grad={want_grad}")


@pytest.mark.parametrize("W,H", EXPOSURE_SIZES)
def test_exposure_bias_gradient(W, H):
    X = sub("exposure")
    q = FS.flat_inputs(W, H, *EXPOSURE)
    image, g = q["r"], q["g"]
    E = (np.eye(4, 3) + 0.1).astype(np.float32).reshape(12)
    want = FS.exposure_bias_grad(g, *EXPOSURE)
    for want_image_grad in (True, False):
        _, dE = X.exposure_backward(gpu(image), gpu(E), gpu(g), want_image_grad=want_image_grad)
        same_bits(dE[9:12], want, f"exposure dL_dE[9..11] {W}x{H} image_grad={want_image_grad}")


@pytest.mark.parametrize("W,H", FS.tile_sizes())
@pytest.mark.parametrize("window", ["gaussian", "reference"])
def test_dssim_l1_sum(W, H, window):
    loss = sub("loss")
    q = FS.tile_inputs(W, H)
    m, r, t = q["m"], q["r"], q["t"]
    pw = loss.PixelWeights(gpu(m))
    for want_grad in (True, False):
        l1, _, _ = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(t), 0.2, window=window, want_grad=want_grad)
        same_bits(l1, FS.dssim_l1_sum(r, t), f"dssim l1_sum {W}x{H} {window} grad={want_grad}")
        l1, _, _ = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(t), 0.2, window=window, want_grad=want_grad, weights=pw)
        same_bits(l1, FS.dssim_l1_sum(r, t, m), f"weighted dssim l1_sum {W}x{H} {window} grad={want_grad}")
