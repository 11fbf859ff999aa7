"""The Pearson-correlation depth loss on the MI355X (include/gsr_depth_corr.h) against its float64 yardstick
(tests/depth_corr_reference.py: centred two-pass moments, never the kernel itself).

Bounds.  Every output is held to K eps32 x (error model), with `worst` = the largest ratio measured on the MI355X over the case matrix
(depth_corr_reference.all_cases: the seven sizes and the six named cases, the adversarial pair among them) and K = 10 x worst, both
in tests/golden/depth_corr_margins.json.  The error models:
    loss   |loss - ref|                                   (the loss lies in [0, 2])
    grad   max_i |g_i - ref_i| / max_i |ref_i|
    fit    |fit_k - ref_k| / (|ref_k| + 1)                per component (rho, s, b, M)
measure_kernels() is the one place that forms the ratios and asserts the exact properties; the tests print the figures before they
assert.  A float32 shortcut in the kernels shows on the adversarial case as a ratio in the hundreds (tests/test_depth_corr_reference.py
holds the yardstick to that).

Invariance on the device: the gradient under t -> 3 t + 1 within 2 K eps32 of max|g|, the loss under t -> -3 t + 1 equal to 2 - loss
within the loss bound.  The test forms those maps in float32, which moves a mapped target t' by up to eps32 / 2 of its magnitude,
and the gradient -- a residual of size sigma_t' sqrt(1 - rho^2) -- by up to ROUNDING = (eps32 / 2) max|t'| / (sigma_t' sqrt(1 - rho^2))
of its largest element.  That is the test's own rounding, not the kernel's: the two maps are held where ROUNDING <= 10 eps32 (7-9.5
on the 37 x 29, block-edge, multi-round, mask-free and negatively correlated cases), and where it is larger (150 on the 3 x 1
case, whose three points correlate to 0.9998; 11 000 on the adversarial pair, |t'| = 33 over a spread of 6e-3) the same two
properties are held under t -> 4 t and t -> -4 t, which float32 forms exactly.

The composition bound (the parameter gradients of a small scene under target -> 2.5 target + 0.3, against the first set) comes from
the same file, and so do the trainer runs over three --depth-seed values: their smallest gap is negative, so the trainer test requires
none (see its docstring)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, lego_camera, pkg, render_kwargs, sub
import depth_corr_reference as R

pytestmark = pytest.mark.gpu
EPS = R.EPS32
MARGINS = os.path.join(ROOT, "tests", "golden", "depth_corr_margins.json")
LAMBDA_DEPTH = "1.0"        # the trainer runs' --lambda-depth: the value tests/test_gpu_aux_grads.py trains the L1 depth term with
PARAM_GRADS = ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity")


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(_dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _margins():
    with open(MARGINS) as fh:
        return json.load(fh)


def _call(c, **kw):
    return sub("loss").depth_corr_loss_and_gradients(_t(c["r"]), _t(c["t"]), _t(c["m"]), **kw)


def make_cases():
    """The case matrix with each case's float64 reference: computed once, shared by the tests, left unchanged."""
    _lib = sub("_lib")
    out = R.all_cases(_lib.DEPTH_CORR_BLOCK_PIXELS, _lib.DEPTH_CORR_MAX_BLOCKS)
    for c in out:
        c["weight"] = 0.7
        c["ref"] = R.closed_form(c["r"], c["t"], c["m"], c["weight"])
        c["degenerate"] = R.moments(c["r"], c["t"], c["m"])["degenerate"]
        if not c["degenerate"] and c["W"] * c["H"] <= 1 << 17:     # autograd = closed form: on the CPU for every case, here where it is cheap
            a_loss, a_grad = R.autograd(c["r"], c["t"], c["m"], c["weight"])
            assert abs(a_loss - c["ref"][0]) <= 1e-10 and np.abs(a_grad - c["ref"][1]).max() <= 1e-10 * np.abs(a_grad).max()
    assert {c["name"] for c in out if c["degenerate"]} >= set(R.DEGENERATE)
    return out


@pytest.fixture(scope="module")
def cases():
    return make_cases()


def _errors(got, ref):
    """(loss, grad, fit) error ratios of one call in units of eps32 x the error model."""
    (loss, grad, fit), (l64, g64, f64) = got, ref
    e_loss = abs(float(loss.item()) - l64) / EPS
    gmax = float(np.abs(g64).max())
    e_grad = float(np.abs(grad.cpu().numpy().astype(np.float64) - g64).max()) / gmax / EPS if gmax > 0 else 0.0
    e_fit = float((np.abs(fit.cpu().numpy().astype(np.float64) - f64) / (np.abs(f64) + 1.0)).max()) / EPS
    return e_loss, e_grad, e_fit


def measure_kernels(cases):
    """{"loss", "grad", "fit"}: the worst error ratio of each output on the matrix, every exact property asserted on every case."""
    L = sub("loss")
    worst = {"loss": 0.0, "grad": 0.0, "fit": 0.0}
    for c in cases:
        name, w = c["name"], c["weight"]
        r, t, m = _t(c["r"]), _t(c["t"]), _t(c["m"])
        loss, grad, fit = L.depth_corr_loss_and_gradients(r, t, m, weight=w)
        assert loss.shape == (1,) and grad.shape == (c["H"], c["W"]) and fit.shape == (4,), name
        assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(fit).all()), name
        e = _errors((loss, grad, fit), c["ref"])
        print(f"{name:22s} loss {float(loss.item()):.7f}  errors (eps32): loss {e[0]:.3f} grad {e[1]:.3f} fit {e[2]:.3f}")
        for k, v in zip(("loss", "grad", "fit"), e):
            worst[k] = max(worst[k], v)
        if c["degenerate"]:                                                                  # exactly (1, zeros, (0, 0, 0, M)), no NaN
            M = float(np.float32(c["ref"][2][3]))
            assert float(loss.item()) == 1.0 and not bool(_bits(grad).any()) and fit.tolist() == [0.0, 0.0, 0.0, M], name
        else:
            assert bool(grad.any()), name
        # two calls: identical bits
        loss2, grad2, fit2 = L.depth_corr_loss_and_gradients(r, t, m, weight=w)
        assert torch.equal(_bits(loss2), _bits(loss)) and torch.equal(_bits(grad2), _bits(grad)) and torch.equal(_bits(fit2), _bits(fit)), name
        # want_grad=False: the same loss and fit bits into the given slots, 1 and 4 floats and no more
        slot = torch.full((3,), float("nan"), device=_dev())
        rows = torch.full((3, 4), float("nan"), device=_dev())
        loss3, none, fit3 = L.depth_corr_loss_and_gradients(r, t, m, weight=w, want_grad=False, loss_out=slot[1:2], fit_out=rows[1])
        assert none is None and loss3.data_ptr() == slot[1:2].data_ptr() and fit3.data_ptr() == rows[1].data_ptr(), name
        assert torch.equal(_bits(slot[1:2]), _bits(loss)) and torch.equal(_bits(rows[1]), _bits(fit)), name
        assert torch.isnan(slot[0]) and torch.isnan(slot[2]) and torch.isnan(rows[0]).all() and torch.isnan(rows[2]).all(), name
        # inputs untouched
        assert torch.equal(_bits(r), _bits(_t(c["r"]))) and torch.equal(_bits(t), _bits(_t(c["t"]))), name
        assert m is None or torch.equal(_bits(m), _bits(_t(c["m"]))), name
        # host arrays give the bits of device tensors; mask=None those of a mask of ones
        hl, hg, hf = L.depth_corr_loss_and_gradients(c["r"], c["t"], c["m"], weight=w)
        assert torch.equal(_bits(hl), _bits(loss)) and torch.equal(_bits(hg), _bits(grad)) and torch.equal(_bits(hf), _bits(fit)), name
        if c["m"] is None:
            ol, og, of = L.depth_corr_loss_and_gradients(r, t, torch.ones_like(r), weight=w)
            assert torch.equal(_bits(ol), _bits(loss)) and torch.equal(_bits(og), _bits(grad)) and torch.equal(_bits(of), _bits(fit)), name
    assert sum(c["m"] is None for c in cases) >= 2
    return worst


def _assert_margins(worst):
    m = _margins()
    for k, w in worst.items():
        assert m[k]["worst"] > 0 and abs(m[k]["K"] - 10.0 * m[k]["worst"]) <= 1e-9 * m[k]["K"], k
        assert w <= m[k]["K"], f"{k}: worst ratio {w:.3f} above K = {m[k]['K']:.3f} (measured {m[k]['worst']:.3f})"


def test_kernels_against_the_yardstick(cases):
    print()
    worst = measure_kernels(cases)
    print("worst error ratios (units of eps32 x error model):", json.dumps(worst))
    _assert_margins(worst)


def test_invariance_under_affine_maps_of_the_target(cases):
    m = _margins()
    K_grad, K_loss = m["grad"]["K"], m["loss"]["K"]
    f32 = np.float32
    print()
    held = {"3 t + 1": 0, "4 t": 0}
    for c in cases:
        if c["degenerate"]:
            continue
        pos, neg = (f32(3.0) * c["t"] + f32(1.0)).astype(f32), (f32(-3.0) * c["t"] + f32(1.0)).astype(f32)
        q = R.moments(c["r"], pos, c["m"])
        rho = q["C"] / np.sqrt(q["Vr"] * q["Vt"])
        rounding = 0.5 * float(np.abs(pos).max()) / np.sqrt(q["Vt"] * (1.0 - rho * rho))       # ROUNDING of the module docstring, in eps32
        label = "3 t + 1" if rounding <= 10.0 else "4 t"
        if label == "4 t":
            pos, neg = f32(4.0) * c["t"], f32(-4.0) * c["t"]
        held[label] += 1
        loss, grad, _ = _call(c, weight=c["weight"])
        gmax = float(grad.abs().max().item())
        l2, g2, _ = _call(dict(c, t=pos), weight=c["weight"])
        e_g = float((g2 - grad).abs().max().item()) / gmax / EPS
        l3, _, _ = _call(dict(c, t=neg), weight=c["weight"], want_grad=False)
        e_l = abs(float(l3.item()) - (2.0 - c["ref"][0])) / EPS
        print(f"{c['name']:22s} (rounding {rounding:8.1f}) {label:8s}: gradient moved by {e_g:.3f} eps32 of max|g| (bound {2 * K_grad:.3f}); "
              f"mirrored loss {float(l3.item()):.7f} against 2 - loss = {2.0 - c['ref'][0]:.7f}: {e_l:.3f} eps32 (bound {K_loss:.3f}); "
              f"loss moved by {abs(float(l2.item()) - float(loss.item())) / EPS:.3f}")
        assert e_g <= 2.0 * K_grad, (c["name"], label)
        assert e_l <= K_loss, (c["name"], label)
    assert held["3 t + 1"] >= 6 and held["4 t"] >= 1, held


# ------------------------------------------------------------------------------------------- composition with the rasterizer
def composition_ratio(scenes, cameras):
    """render -> depth_corr_loss_and_gradients -> backward(dL_ddepth_image=...) on a small scene at 128 x 96, twice: with a noisy
    multiple of the render's own inverse depth as the target, and with 2.5 target + 0.3.  Returns the worst
    max|g2 - g1| / max|g1| over PARAM_GRADS in units of eps32 (the backward's float atomics are in it), and the first set."""
    gsr = pkg()
    W, H = 128, 96
    sc = scenes.synthetic_scene(3000, 0.05, 0.6, 7)
    cam = lego_camera(cameras, 0, W, H)
    kw = render_kwargs(sc, cam)
    _, dep, buf = gsr.render_gaussians(**kw)
    dep = dep.reshape(H, W)
    d = dep.cpu().numpy()
    assert (d > 0).mean() > 0.2
    rng = np.random.default_rng(3)
    target = np.where(d > 0, d * (1.0 + 0.2 * rng.normal(0, 1, d.shape)) + 0.05 * rng.normal(0, 1, d.shape) + 0.5, 0.0).astype(np.float32)
    mask = (d > 0).astype(np.float32)
    sets = []
    for tg in (target, np.where(d > 0, np.float32(2.5) * target + np.float32(0.3), 0.0).astype(np.float32)):
        loss, grad, fit = gsr.loss.depth_corr_loss_and_gradients(dep, tg, mask, weight=0.1)
        b = backward_kwargs(sc, cam, kw, buf, None)
        b["geom_buffer"] = dict(b["geom_buffer"], depths=buf["depths"])
        g = gsr.backward(**b, dL_ddepth_image=grad)
        sets.append(({k: g[k].detach().cpu().numpy().astype(np.float64) for k in PARAM_GRADS}, float(loss.item()), fit.tolist()))
    (g1, l1, f1), (g2, l2, f2) = sets
    ratios = {k: float(np.abs(g2[k] - g1[k]).max() / np.abs(g1[k]).max() / EPS) for k in PARAM_GRADS}
    print(f"\ncomposition: loss {l1:.6f} / {l2:.6f}, fit {f1} / {f2}; parameter gradients moved by (eps32 of max|g|): {json.dumps(ratios)}")
    return max(ratios.values()), g1


def test_composition_with_the_backward_is_blind_to_scale_and_shift(scenes, cameras):
    worst, g1 = composition_ratio(scenes, cameras)
    for k in PARAM_GRADS:
        assert np.isfinite(g1[k]).all() and np.abs(g1[k]).max() > 0, k
    m = _margins()["composition"]
    assert m["worst"] > 0 and abs(m["K"] - 10.0 * m["worst"]) <= 1e-9 * m["K"]
    assert worst <= m["K"], f"composition: {worst:.1f} above K = {m['K']:.1f} (measured {m['worst']:.1f})"


# ------------------------------------------------------------------------------------------- the trainer on the hidden scene
def trainer_run(tmp, label, seed, *extra):
    """One run of examples/train.py in hidden-scene mode at 100 x 100, 8 views, 300 iterations, --depth-noise 1: its summary."""
    log = os.path.join(tmp, f"{label}.jsonl")
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train.py"), "--size", "100", "--views", "8", "--iterations", "300", "--depth-noise", "1",
           "--depth-seed", str(seed), "--print-interval", "1000", "--log", log, *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    summary = [r for r in map(json.loads, open(log)) if r["record"] == "summary"][0]
    assert all(summary["parameters_finite"].values())
    for k in ("train_depth_l1_mean", "train_depth_l1_clean_mean", "train_depth_corr_mean", "train_psnr_mean"):
        assert np.isfinite(summary[k]), k
    fit = np.asarray(summary["train_depth_fit"])
    assert fit.shape == (8, 2) and np.isfinite(fit).all()
    return summary


def trainer_trio(tmp, seed):
    """{"l1", "pearson", "none"}: the summaries of the three runs on the same perturbed targets."""
    return {"l1": trainer_run(tmp, f"l1_{seed}", seed, "--lambda-depth", LAMBDA_DEPTH, "--depth-loss", "l1"),
            "pearson": trainer_run(tmp, f"pearson_{seed}", seed, "--lambda-depth", LAMBDA_DEPTH, "--depth-loss", "pearson"),
            "none": trainer_run(tmp, f"none_{seed}", seed, "--lambda-depth", "0")}


def test_trainer_runs_with_either_depth_loss_on_relative_depth_targets(tmp_path):
    """The claim this test was to hold -- --depth-loss pearson ends with a lower clean depth L1 than --depth-loss l1 on the same
    perturbed targets -- is FALSE for this setup (hidden scene, 100 x 100, 8 views, 300 iterations, --lambda-depth 1, --depth-noise 1),
    measured on the MI355X over --depth-seed 0, 1, 2 (tests/golden/depth_corr_margins.json): clean depth L1 0.0904 / 0.0778 / 0.0571
    with l1, 0.0732 / 0.0729 / 0.0731 with pearson -- gaps +0.0173, +0.0050, -0.0160 -- and 0.0223 with no depth term at all.  The
    Pearson term does what it is for (rho 0.956 against 0.63-0.77 with l1 and 0.69 with no depth term; its result does not depend on
    the perturbation's seed, the L1's does), but at this weight and length either depth term costs absolute depth and 1.1-1.9 dB.
    Nothing was tuned.  So, as the issue asks for this outcome, the test asserts only that the three runs end finite with the summary
    fields present (trainer_run), and prints the figures; the margins file records that the claim does not hold."""
    m = _margins()["trainer"]
    runs = trainer_trio(str(tmp_path), 0)
    print()
    for k, s in runs.items():
        print(f"--depth-noise 1, {k:8s}: clean depth L1 {s['train_depth_l1_clean_mean']:.6f}, depth L1 as given {s['train_depth_l1_mean']:.6f}, "
              f"rho {s['train_depth_corr_mean']:.4f}, PSNR {s['train_psnr_mean']:.2f} dB")
    gap = runs["l1"]["train_depth_l1_clean_mean"] - runs["pearson"]["train_depth_l1_clean_mean"]
    print(f"gap {gap:.6f}; measured over seeds {m['seeds']}: {m['gaps']}")
    assert len(m["gaps"]) == 3 and m["claim_holds"] == (min(m["gaps"]) > 0) and m["claim_holds"] is False and m["required_gap"] is None
