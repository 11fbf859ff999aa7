"""The weighted colour loss (include/gsr_weighted_loss.h) on the MI355X, against the float64 definition of
tests/weighted_loss_reference.py: the weight total, L1 sum, SSIM sum and pixel_grad for both windows and lambda in {0, 0.2, 1}, at
sizes chosen for the 32 x 16 tile and one 800 x 800, under seven kinds of weight image -- ones, random binary 8 x 8 blocks, smooth
floats in [0, 2], a rectangular hole, a single weighted pixel at (31, 15) and at (32, 16) (the last pixel of one tile, the first of
the next) and all zeros, which must give exact zeros.  Then the contracts: all-ones weights against the unweighted entry points,
4 m against m, exact zeros outside the weights' 5-pixel reach, an occluder under a grown mask invisible bit for bit, bit-identical
repeat calls, untouched canary words, lambda = 0 against the weighted L1 entry bit for bit, and the trainer with --occluders with
and without --mask-occluders.

Tripwires: 10 x the largest margin measured on an MI355X (tests/golden/weighted_loss_margins.json, written by
tools/weighted_loss_margins.py from this file's own case list), the gradient's never above the project's ceiling of
1e-3 max|g_f64|.  The trainer test's required gaps are half the smallest gap measured over three --occluder-seed values."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import weighted_loss_reference as WR
from conftest import ROOT, sub
from test_gpu_dssim import gpu, images

pytestmark = pytest.mark.gpu

MARGINS = os.path.join(ROOT, "tests", "golden", "weighted_loss_margins.json")
GRAD_CEILING = 1e-3                                    # the project's ceiling on max|dg| / max|g_f64|, whatever was measured
SIZES = [(1, 1), (5, 9), (17, 33), (31, 17), (33, 15), (64, 48), (97, 61), (200, 300)]   # (W, H)
KINDS = ["ones", "blocks", "smooth", "hole", "pixel_31_15", "pixel_32_16", "zeros"]
WINDOWS = ["gaussian", "reference"]
LAMBDAS = [0.0, 0.2, 1.0]


def weight_image(kind, W, H):
    """The (H, W) float32 weights of a case, or None where the size has no such pixel."""
    rng = np.random.default_rng(104729 * W + H)
    if kind == "ones":
        return np.ones((H, W), np.float32)
    if kind == "zeros":
        return np.zeros((H, W), np.float32)
    if kind == "blocks":
        b = rng.integers(0, 2, ((H + 7) // 8, (W + 7) // 8)).astype(np.float32)
        return np.ascontiguousarray(np.kron(b, np.ones((8, 8), np.float32))[:H, :W])
    if kind == "smooth":
        yy, xx = np.mgrid[0:H, 0:W]
        a, p = rng.uniform(0.1, 0.5, 4), rng.uniform(0, 6.28, 2)
        return (1.0 + np.sin(a[0] * xx + a[1] * yy + p[0]) * np.cos(a[2] * xx - a[3] * yy + p[1])).astype(np.float32)
    if kind == "hole":
        m = np.ones((H, W), np.float32)
        m[H // 4:H // 4 + max(1, H // 3), W // 3:W // 3 + max(1, W // 4)] = 0.0
        return m
    x, y = (31, 15) if kind == "pixel_31_15" else (32, 16)
    if x >= W or y >= H:
        return None
    m = np.zeros((H, W), np.float32)
    m[y, x] = 1.0
    return m


CASES = [(W, H, k) for W, H in SIZES for k in KINDS if weight_image(k, W, H) is not None] + [(800, 800, "blocks")]


def _margins():
    with open(MARGINS) as f:
        return json.load(f)


def f64(a):
    return torch.as_tensor(a, dtype=WR.F64).cuda()


@functools.lru_cache(maxsize=4)
def reference(W, H, kind, window):
    """The float64 outputs of a case, computed once and shared by its three lambdas: the gradient is linear in lambda."""
    r, t = images(W, H)
    m = weight_image(kind, W, H)
    x, y, mm = f64(r), f64(t), f64(m)
    return {"g0": WR.pixel_grad(x, y, mm, 0.0, window).cpu(), "g1": WR.pixel_grad(x, y, mm, 1.0, window).cpu(),
            "l1": float(WR.l1_sum(x, y, mm)), "ssim": float(WR.ssim_sum(x, y, mm, window)), "total": float(mm.sum())}


def run(r, t, m, lam, window, want_grad=True):
    loss = sub("loss")
    pw = m if isinstance(m, loss.PixelWeights) else loss.PixelWeights(gpu(m))
    l1, ss, g = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(t), lam, window=window, want_grad=want_grad, weights=pw)
    torch.cuda.synchronize()
    return float(l1.item()), float(ss.item()), (g.cpu().double() if g is not None else None), float(pw.total.item())


def case_margins(W, H, kind, window, lam):
    """The four errors of a case as the tripwires measure them: max|dg| / max|g_f64|, |dssim_sum| / M, and relative for the L1 sum and
    M.  With M = 0 the float64 outputs are zeros and the errors are the absolute values of the kernels' outputs ("zero": True)."""
    ref = reference(W, H, kind, window)
    l1, ss, g, total = run(*images(W, H), weight_image(kind, W, H), lam, window)
    gr = (1.0 - lam) * ref["g0"] + lam * ref["g1"]
    if ref["total"] == 0.0:
        return {"zero": True, "grad": float(g.abs().max()), "ssim": abs(ss), "l1": abs(l1), "total": abs(total)}
    return {"zero": False, "grad": float((g - gr).abs().max() / gr.abs().max()), "ssim": abs(ss - ref["ssim"]) / ref["total"],
            "l1": abs(l1 - ref["l1"]) / max(ref["l1"], 1e-30), "total": abs(total - ref["total"]) / ref["total"]}


@pytest.mark.parametrize("W,H,kind", CASES)
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("lam", LAMBDAS)
def test_against_the_float64_definition(W, H, kind, window, lam):
    m = case_margins(W, H, kind, window, lam)
    print(json.dumps({"W": W, "H": H, "kind": kind, "window": window, "lambda": lam, **m}))
    measured = _margins()["kernels"]
    tol = {k: 10.0 * measured[k] for k in ("grad", "ssim", "l1", "total")}
    tol["grad"] = min(tol["grad"], GRAD_CEILING)
    assert 0.0 < measured["grad"] <= GRAD_CEILING                              # above the ceiling is a bug, not a margin
    if m["zero"]:
        assert m["grad"] == m["ssim"] == m["l1"] == m["total"] == 0.0, m      # exact zeros in every output
    else:
        assert all(m[k] <= tol[k] for k in tol), (m, tol)


@pytest.mark.parametrize("W,H", [(800, 800), (97, 61), (33, 15), (1, 1)])
@pytest.mark.parametrize("window", WINDOWS)
def test_all_ones_is_the_unweighted_call(W, H, window):
    """Gradient within 1e-5 max|g| (one more rounding of the scale factor, then a linear convolution), sums within 1e-6 relative."""
    loss = sub("loss")
    r, t = images(W, H)
    ones = np.ones((H, W), np.float32)
    for lam in (0.2, 1.0):
        l1, ss, g, total = run(r, t, ones, lam, window)
        l1u, ssu, gu = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(t), lam, window=window)
        gu = gu.cpu().double()
        assert total == W * H
        assert float((g - gu).abs().max()) <= 1e-5 * float(gu.abs().max())
        assert abs(l1 - float(l1u.item())) <= 1e-6 * float(l1u.item()) and abs(ss - float(ssu.item())) <= 1e-6 * abs(float(ssu.item()))
    s, g = loss.l1_loss_and_gradients(gpu(r), gpu(t), 0.2, weights=gpu(ones))     # a bare tensor: its total is computed in the call
    su, gu = loss.l1_loss_and_gradients(gpu(r), gpu(t), 0.2)
    assert float((g - gu).abs().max()) <= 1e-5 * float(gu.abs().max())
    assert abs(float(s.item()) - float(su.item())) <= 1e-6 * float(su.item())


@pytest.mark.parametrize("W,H,kind", [(800, 800, "smooth"), (97, 61, "smooth"), (33, 15, "blocks")])
def test_four_times_the_weights_is_the_same_loss(W, H, kind):
    """4 m against m: the gradient within 1e-6 max|g|, l1_sum exactly 4 x.  Scaling by a power of two is exact in IEEE arithmetic, and
    every product the kernels form with M or m keeps it exact, so on the MI355X all outputs were in fact bit-equal (gradient equal,
    both sums exactly 4 x); the printed line says which it was."""
    r, t = images(W, H)
    m = weight_image(kind, W, H)
    l1, ss, g, total = run(r, t, m, 0.2, "gaussian")
    l1k, ssk, gk, totalk = run(r, t, 4.0 * m, 0.2, "gaussian")
    print(f"\n4 m against m at {W} x {H}: gradient bit-equal {torch.equal(g, gk)}, max|dg| / max|g| {float((g - gk).abs().max() / g.abs().max()):.3e}, "
          f"ssim_sum exactly 4 x: {ssk == 4.0 * ss}")
    assert totalk == 4.0 * total and l1k == 4.0 * l1
    assert float((g - gk).abs().max()) <= 1e-6 * float(g.abs().max())
    assert abs(ssk - 4.0 * ss) <= 1e-6 * abs(4.0 * ss)


@pytest.mark.parametrize("W,H,kind", [(200, 300, "blocks"), (97, 61, "hole"), (64, 48, "pixel_31_15"), (64, 48, "pixel_32_16")])
@pytest.mark.parametrize("window", WINDOWS)
def test_exact_zeros_outside_the_reach_of_the_weights(W, H, kind, window):
    r, t = images(W, H)
    m = weight_image(kind, W, H)
    reach = WR.reach(torch.as_tensor(m))
    assert 0 < int(reach.sum())
    g = run(r, t, m, 0.2, window)[2]
    assert bool((g[~reach] == 0).all())
    ring = reach & ~torch.as_tensor(m > 0)
    assert float(g[ring].abs().max()) > 0.0                               # a weight-0 pixel inside a weighted pixel's window gets SSIM gradient
    assert bool((run(r, t, m, 0.0, window)[2][ring] == 0).all())           # ... and no L1 gradient


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("W,H", [(800, 800), (97, 61)])
@pytest.mark.parametrize("window", WINDOWS)
def test_an_occluder_under_a_grown_mask_is_invisible(W, H, window):
    """Weights 0 on a rectangle and within 5 pixels of it (PixelWeights(dilate=5)): l1_sum, ssim_sum and pixel_grad are, bit for bit,
    those of the clean target under the same weights -- also the signs of their zeros.  The rectangle straddles tile borders."""
    loss = sub("loss")
    r, t = images(W, H)
    y0, y1, x0, x1 = H // 5, H // 5 + H // 3, W // 4 + 3, W // 4 + 3 + W // 3
    occluded = t.copy()
    occluded[y0:y1, x0:x1] = (1.0, 0.0, 1.0)
    tight = weight_image("smooth", W, H) + np.float32(0.01)
    tight[y0:y1, x0:x1] = 0.0
    pw = loss.PixelWeights(gpu(tight), dilate=5)
    want = WR.dilate_zeros(torch.as_tensor(tight), 5)
    assert torch.equal(pw.weights.cpu(), want) and int((want == 0).sum()) == (y1 - y0 + 10) * (x1 - x0 + 10)
    for lam in (0.2, 1.0):
        a = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(occluded), lam, window=window, weights=pw)
        b = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(t), lam, window=window, weights=pw)
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b))
    a = loss.l1_loss_and_gradients(gpu(r), gpu(occluded), weights=pw)
    b = loss.l1_loss_and_gradients(gpu(r), gpu(t), weights=pw)
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b))
    tight_pw = loss.PixelWeights(gpu(tight))                               # the rectangle's own mask, not grown: its rim still shows
    a = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(occluded), 0.2, window=window, weights=tight_pw)
    b = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(t), 0.2, window=window, weights=tight_pw)
    assert not torch.equal(a[2], b[2]) and torch.equal(a[0], b[0])


@pytest.mark.parametrize("W,H", [(800, 800), (97, 61)])
def test_two_calls_give_the_same_bits(W, H):
    loss = sub("loss")
    r, t = images(W, H)
    m = gpu(weight_image("smooth", W, H))
    pa, pb = loss.PixelWeights(m), loss.PixelWeights(m)
    assert torch.equal(bits(pa.total), bits(pb.total))
    a = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(t), 0.2, weights=pa)
    b = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(t), 0.2, weights=pb)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    a = loss.l1_loss_and_gradients(gpu(r), gpu(t), weights=pa)
    b = loss.l1_loss_and_gradients(gpu(r), gpu(t), weights=m)             # a bare tensor: the same total, computed in the call
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("W,H", [(800, 800), (33, 15), (5, 9), (1, 1)])
def test_canaries_after_pixel_grad_workspaces_and_sum_words(W, H):
    _lib, host = sub("_lib"), sub("_host")
    L = _lib.lib()
    r, t = images(W, H)
    rd, td, md = gpu(r), gpu(t), gpu(weight_image("smooth", W, H))
    stream = host.stream_ptr(rd.device)
    n, pad = H * W * 3, 4096
    sum_b, dssim_b = int(L.gsr_weight_total_workspace_bytes(W, H)), int(L.gsr_weighted_dssim_workspace_bytes(W, H))
    sums = torch.zeros(12, device="cuda")                                  # M in slot 1, the L1 call's sum in 5, the D-SSIM call's in 8 and 10
    for call in ("total", "l1", "dssim"):
        need = dssim_b if call == "dssim" else sum_b
        gbuf = torch.full((n + pad,), 1234.5, device="cuda")
        wbuf = torch.full((need // 4 + pad,), -77.25, device="cuda")
        if call == "total":
            rc = L.gsr_weight_total(host.ptr(md), W, H, host.ptr(sums[1:]), host.ptr(wbuf), need, stream)
        elif call == "l1":
            rc = L.gsr_weighted_l1_loss_grad(host.ptr(rd), host.ptr(td), host.ptr(md), host.ptr(sums[1:]), host.ptr(gbuf), host.ptr(sums[5:]), W, H,
                                             1.0, host.ptr(wbuf), need, stream)
        else:
            rc = L.gsr_weighted_l1_dssim_loss_grad(host.ptr(rd), host.ptr(td), host.ptr(md), host.ptr(sums[1:]), host.ptr(gbuf), host.ptr(sums[8:]),
                                                   host.ptr(sums[10:]), W, H, 0.2, 1, host.ptr(wbuf), need, stream)
        torch.cuda.synchronize()
        assert rc == 0, call
        assert bool((wbuf[need // 4:] == -77.25).all()), call
        if call != "total":
            assert bool((gbuf[n:] == 1234.5).all()) and bool(torch.isfinite(gbuf[:n]).all()), call
    assert bool((sums[[0, 2, 3, 4, 6, 7, 9, 11]] == 0).all()) and bool((sums[[1, 5, 8, 10]] != 0).all()), sums


@pytest.mark.parametrize("W,H", [(800, 800), (17, 33), (1, 1)])
@pytest.mark.parametrize("window", WINDOWS)
def test_lambda_zero_is_the_weighted_l1_gradient_bit_for_bit(W, H, window):
    loss = sub("loss")
    r, t = images(W, H)
    t[0, 0] = r[0, 0]                                                      # sign(0) = +1 on both paths
    pw = loss.PixelWeights(gpu(weight_image("hole" if W > 1 else "ones", W, H) * weight_image("smooth", W, H)))
    s, want = loss.l1_loss_and_gradients(gpu(r), gpu(t), 0.0, weights=pw)
    l1, _, got = loss.l1_dssim_loss_and_gradients(gpu(r), gpu(t), 0.0, window=window, weights=pw)
    assert torch.equal(bits(got), bits(want))
    assert float(l1.item()) == pytest.approx(float(s.item()), rel=1e-6)


# ------------------------------------------------------------------------------------------- the trainer on Lego
def trainer_run(tmp, label, *extra):
    """One run of examples/train.py on the eight Lego views, 300 iterations, --lambda-dssim 0.2: its summary record."""
    log = os.path.join(tmp, f"{label}.jsonl")
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train.py"), "--dataset", os.path.join(ROOT, "data", "lego"), "--views", "8",
           "--iterations", "300", "--lambda-dssim", "0.2", "--print-interval", "100", "--log", log, *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    recs = [json.loads(l) for l in open(log)]
    summary = [r for r in recs if r["record"] == "summary"][0]
    curve = np.concatenate([np.asarray(r["l1"], np.float64) for r in recs if r["record"] == "loss"])
    assert len(curve) == 300 and np.isfinite(curve).all() and all(summary["parameters_finite"].values())
    return dict(summary, final_loss=float(curve[-50:].mean()))


def test_trainer_masking_the_occluders_wins_on_the_clean_targets(tmp_path):
    m = _margins()["trainer"]
    occ = ("--occluders", "3", "--occluder-seed", "0")
    plain = trainer_run(str(tmp_path), "plain", *occ)
    masked = trainer_run(str(tmp_path), "masked", *occ, "--mask-occluders")
    psnr_gap, l1_gap = masked["clean_psnr_mean"] - plain["clean_psnr_mean"], plain["clean_l1_mean"] - masked["clean_l1_mean"]
    print(f"\n--occluders 3: clean PSNR {plain['clean_psnr_mean']:.2f} -> {masked['clean_psnr_mean']:.2f} dB with --mask-occluders (gap {psnr_gap:.2f}, "
          f"required {m['required_psnr_gap']:.2f}); clean L1 {plain['clean_l1_mean']:.5f} -> {masked['clean_l1_mean']:.5f} (gap {l1_gap:.5f}, "
          f"required {m['required_l1_gap']:.5f})")
    assert abs(m["required_psnr_gap"] - 0.5 * min(m["psnr_gaps"])) <= 1e-12 and abs(m["required_l1_gap"] - 0.5 * min(m["l1_gaps"])) <= 1e-12
    assert m["required_psnr_gap"] > 0 and m["required_l1_gap"] > 0
    assert psnr_gap >= m["required_psnr_gap"]
    assert l1_gap >= m["required_l1_gap"]
    for key in ("train_weighted_l1_mean", "train_weighted_psnr_mean", "train_weighted_ssim_mean", "train_views_weighted"):
        assert key in masked and key not in plain, key
    assert len(masked["train_views_weighted"]) == 8 and "clean_ssim_mean" in plain and "clean_ssim_mean" in masked
    assert masked["train_weighted_psnr_mean"] > masked["train_psnr_mean"]     # the rectangles it did not fit no longer count against it


def test_trainer_with_an_all_ones_mask_dir_is_no_worse_than_without(tmp_path):
    """--mask-dir of all-255 PNGs against no mask: within the spread the plain occluded run showed from seed to seed."""
    from PIL import Image
    m = _margins()["trainer"]
    masks = tmp_path / "masks"
    masks.mkdir()
    for k in range(8):
        Image.fromarray(np.full((800, 800), 255, np.uint8)).save(masks / f"r_{k}.png")
    plain = trainer_run(str(tmp_path), "none")
    ones = trainer_run(str(tmp_path), "ones", "--mask-dir", str(masks))
    print(f"\nall-ones --mask-dir: training PSNR {plain['train_psnr_mean']:.2f} / {ones['train_psnr_mean']:.2f} dB (allowed -{m['plain_psnr_spread']:.2f}); "
          f"training L1 {plain['train_l1_mean']:.5f} / {ones['train_l1_mean']:.5f} (allowed +{m['plain_l1_spread']:.5f})")
    assert abs(m["plain_psnr_spread"] - (max(m["plain_clean_psnr"]) - min(m["plain_clean_psnr"]))) <= 1e-12
    assert abs(m["plain_l1_spread"] - (max(m["plain_clean_l1"]) - min(m["plain_clean_l1"]))) <= 1e-12
    assert ones["train_psnr_mean"] >= plain["train_psnr_mean"] - m["plain_psnr_spread"]
    assert ones["train_l1_mean"] <= plain["train_l1_mean"] + m["plain_l1_spread"]
    assert ones["train_weighted_psnr_mean"] == pytest.approx(ones["train_psnr_mean"], abs=1e-3)      # all ones: the weighted scores are the plain ones
    assert ones["train_weighted_l1_mean"] == pytest.approx(ones["train_l1_mean"], rel=1e-5)
