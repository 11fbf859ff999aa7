"""The model of the fixed-order sum (tests/fixed_order_sum.py) held to itself on the CPU: one element comes back unchanged, sums of
small integers are exact, and on the seeded inputs of the GPU tests (tests/test_gpu_fixed_order_sum.py) its result differs in bits
from a sequential sum and from np.sum -- the condition that lets those tests tell one order of additions from another."""
import os
import re

import numpy as np
import pytest

import fixed_order_sum as FS
from exposure_reference import case_sizes
from conftest import ROOT, sub

_lib = sub("_lib")
EXPOSURE_SIZES = case_sizes(_lib.EXPOSURE_BLOCK_PIXELS, _lib.EXPOSURE_MAX_BLOCKS)


@pytest.mark.parametrize("dtype", [FS.F32, FS.F64])
@pytest.mark.parametrize("order", ["pairwise", "serial"])
def test_one_element_comes_back_unchanged(dtype, order):
    x = dtype(-1.2345678901234567e-3)
    for lane in (0, 1, 63, 64, 255):
        lanes = np.zeros(FS.THREADS, dtype)
        lanes[lane] = x
        assert FS.bits(FS.block_sum(lanes, order)) == FS.bits(x)
    for n, at in ((1, 0), (257, 256), (1000, 511)):
        rec = np.zeros(n, dtype)
        rec[at] = x
        assert FS.bits(FS.finish(rec, order)) == FS.bits(x)
    w = np.zeros((1, 1), FS.F32)
    w[0, 0] = FS.F32(x)
    assert FS.bits(FS.weight_total(w)) == FS.bits(FS.F32(x))


@pytest.mark.parametrize("order", ["pairwise", "serial"])
def test_small_integers_sum_exactly(order):
    rng = np.random.default_rng(1)
    for dtype in (FS.F32, FS.F64):
        lanes = rng.integers(-1000, 1000, (5, FS.THREADS)).astype(dtype)
        assert np.array_equal(FS.block_sum(lanes, order), lanes.astype(np.int64).sum(-1).astype(dtype))
        rec = rng.integers(-1000, 1000, 777).astype(dtype)
        assert FS.finish(rec, order) == dtype(rec.astype(np.int64).sum())
    assert FS.block_sum(lanes.astype(FS.F32), order, acc=FS.F64).dtype == FS.F64     # float32 butterflies, float64 wave sums
    for W, H in FS.flat_sizes():
        m = rng.integers(0, 8, (H, W)).astype(FS.F32)
        r, t = rng.integers(-8, 8, (2, H, W, 3)).astype(FS.F32)
        assert FS.weight_total(m) == m.astype(np.int64).sum()
        assert FS.weighted_l1_sum(r, t, m) == (m[:, :, None] * np.abs(r - t)).astype(np.int64).sum()
        assert np.array_equal(FS.exposure_bias_grad(r, _lib.EXPOSURE_BLOCK_PIXELS, _lib.EXPOSURE_MAX_BLOCKS), r.astype(np.int64).sum((0, 1)))
    for W, H in FS.tile_sizes():
        m = rng.integers(0, 8, (H, W)).astype(FS.F32)
        r, t = rng.integers(-8, 8, (2, H, W, 3)).astype(FS.F32)
        assert FS.dssim_l1_sum(r, t) == np.abs(r - t).astype(np.int64).sum()
        assert FS.dssim_l1_sum(r, t, m) == (m[:, :, None] * np.abs(r - t)).astype(np.int64).sum()


def test_the_models_constants_are_the_kernels():
    """dssim.hip keeps its flat kernels' block size and grid cap to itself (no _lib.py constant), so the model's copy is held to the source."""
    csrc = os.path.join(ROOT, "3dgs-native_amd", "csrc")
    with open(os.path.join(csrc, "dssim.hip")) as f:
        flat = f.read()
    with open(os.path.join(csrc, "dssim_window.h")) as f:
        tx, ty, nt = (int(v) for v in re.search(r"constexpr int TX = (\d+), TY = (\d+), NT = (\d+);", f.read()).groups())
    assert (tx, ty, nt) == (FS.TILE_W, FS.TILE_H, FS.THREADS)
    assert int(re.search(r"constexpr int SUM_BLOCK_PIXELS = (\d+) \* NT;", flat).group(1)) * nt == FS.BLOCK_PIXELS
    assert int(re.search(r"constexpr int MAX_SUM_BLOCKS = (\d+);", flat).group(1)) == FS.WEIGHTED_MAX_BLOCKS
    assert FS.BLOCK_PIXELS == _lib.EXPOSURE_BLOCK_PIXELS


def test_the_two_wave_orders_differ():
    w = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24], FS.F32)     # serial loses every small term, pairwise keeps two of them
    assert FS.four_waves(w, "serial") == 1.0 and FS.four_waves(w, "pairwise") > 1.0


@pytest.mark.parametrize("W,H", [s for s in FS.flat_sizes() + EXPOSURE_SIZES if s[0] * s[1] > FS.GROUP])
def test_flat_models_differ_from_other_orders_on_the_gpu_tests_inputs(W, H):
    """From 5 x 7 up.  1 x 1, 3 x 1 and 4 x 1 are exempt: up to three terms every order adds alike, and the one group of 4 x 1 is added
    by one lane in sequence in the exposure sums."""
    assert FS.flat_orders_show(FS.flat_inputs(W, H, _lib.EXPOSURE_BLOCK_PIXELS, _lib.EXPOSURE_MAX_BLOCKS), _lib.EXPOSURE_BLOCK_PIXELS, _lib.EXPOSURE_MAX_BLOCKS)


@pytest.mark.parametrize("W,H", [s for s in FS.tile_sizes() if s[0] * s[1] > 1])
def test_tile_model_differs_from_other_orders_on_the_gpu_tests_inputs(W, H):
    q = FS.tile_inputs(W, H)
    assert FS.order_shows(FS.dssim_l1_sum(q["r"], q["t"]), np.abs(q["r"] - q["t"]))
    assert FS.order_shows(FS.dssim_l1_sum(q["r"], q["t"], q["m"]), q["m"][:, :, None] * np.abs(q["r"] - q["t"]))
