"""Per-view exposure compensation on the MI355X (include/gsr_exposure.h) against its float64 yardstick (tests/exposure_reference.py).

Bounds.  Every kernel is held to K eps32 x (error model), with `worst` = the largest ratio measured on the MI355X on the case
matrix below and K = 10 x worst, both in tests/golden/exposure_margins.json.  The error models:
    apply          |c'_j - ref| / (sum_i |c_i A_ij| + |b_j|)              per element
    backward_image |dL/dc_i - ref| / sum_j |A_ij g_j|                     per element
    backward_E     |dL/dE_k - ref| / (sum over pixels of |term_k|)        per element of E.  No sqrt(P): the sums are a tree (4 pixels per
                   lane and round, a 64-lane butterfly, 4 waves, up to 4 records per finishing lane, the same tree again), whose
                   rounding error is at most (depth + 1) eps32 sum|terms| with depth <= 27 whatever P is; rounds beyond the first add
                   one level per GSR_EXPOSURE_MAX_BLOCKS x GSR_EXPOSURE_BLOCK_PIXELS pixels (256 at the 2^28 limit).
    adam           |x - ref| / (|ref| + sum of the learning rates so far) for E (its travel is at most the sum of the rates),
                   / max_t |g_t| for m, / max_t g_t^2 for v, over 1, 2 and 1 000 steps of a fixed gradient sequence.
measure_kernels() / measure_adam() are the one place that forms the ratios; the tests print the figures before they assert.

The trainer test's required gaps are half the smallest gap measured over three --exposure-seed values, from the same file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg, render_kwargs, sub
import exposure_reference as R

pytestmark = pytest.mark.gpu
EPS = R.EPS32
MARGINS = os.path.join(ROOT, "tests", "golden", "exposure_margins.json")


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(_dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _margins():
    with open(MARGINS) as fh:
        return json.load(fh)


def _ratio(got, ref, mag):
    nz = mag > 0
    assert (got[~nz] == 0).all()                       # no term: the result is zero exactly
    return float((np.abs(got.astype(np.float64) - ref)[nz] / mag[nz]).max() / EPS) if nz.any() else 0.0


@pytest.fixture(scope="module")
def cases():
    _lib = sub("_lib")
    out = []
    for k, (W, H) in enumerate(R.case_sizes(_lib.EXPOSURE_BLOCK_PIXELS, _lib.EXPOSURE_MAX_BLOCKS)):
        c = R.make_case(W, H, 100 + k)
        c["apply"] = R.apply_f64(c["image"], c["E"])
        c["closed"] = R.backward_closed(c["image"], c["E"], c["g"])
        if W * H <= 1 << 19:                           # autograd = closed form: on the CPU for every case, here where it is cheap
            a_img, a_E = R.backward_autograd(c["image"], c["E"], c["g"])
            assert np.allclose(a_img, c["closed"][0], rtol=1e-12, atol=0) and (np.abs(a_E - c["closed"][1]) <= 1e-12 * c["closed"][3]).all()
        out.append(c)
    return out


def measure_kernels(cases):
    """{"apply", "backward_image", "backward_E"}: the worst error ratio of each kernel on the matrix, every exact property asserted."""
    X, _lib = sub("exposure"), sub("_lib")
    worst = {"apply": 0.0, "backward_image": 0.0, "backward_E": 0.0}
    ident = _t(X.IDENTITY)
    for c in cases:
        name = f"{c['W']}x{c['H']}"
        img, E, g = _t(c["image"]), _t(c["E"]), _t(c["g"])
        # ---- apply ----
        out = X.apply_exposure(img, E)
        assert out.shape == img.shape and out.data_ptr() != img.data_ptr(), name
        worst["apply"] = max(worst["apply"], _ratio(out.cpu().numpy(), *c["apply"]))
        same = X.apply_exposure(img, ident)
        assert torch.equal(_bits(same), _bits(img + 0.0)), name                              # identity: bit for bit (-0 comes back +0)
        neg0 = np.signbit(c["image"]) & (c["image"] == 0)
        assert not np.signbit(same.cpu().numpy()[neg0]).any(), name
        inplace = img.clone()
        ver = inplace._version
        assert X.apply_exposure(inplace, E, out=inplace) is inplace and inplace._version > ver, name
        assert torch.equal(_bits(inplace), _bits(out)), name                                 # in place = out of place
        # ---- backward ----
        d_ref, dE_ref, mag_img, mag_E = c["closed"]
        d_img, dE = X.exposure_backward(img, E, g)
        assert d_img.data_ptr() != g.data_ptr() and dE.shape == (12,), name
        worst["backward_image"] = max(worst["backward_image"], _ratio(d_img.cpu().numpy(), d_ref, mag_img))
        worst["backward_E"] = max(worst["backward_E"], _ratio(dE.cpu().numpy(), dE_ref, mag_E))
        d2, dE2 = X.exposure_backward(img, E, g)
        assert torch.equal(_bits(d2), _bits(d_img)) and torch.equal(_bits(dE2), _bits(dE)), name   # two calls: identical bits
        gi = g.clone()
        ver = gi._version
        d3, dE3 = X.exposure_backward(img, E, gi, out=gi)
        assert d3 is gi and gi._version > ver, name                                          # the in-place write is reported
        assert torch.equal(_bits(gi), _bits(d_img)) and torch.equal(_bits(dE3), _bits(dE)), name    # in place = out of place
        row = torch.full((3, 12), float("nan"), device=_dev())
        none, dE4 = X.exposure_backward(img, E, g, want_image_grad=False, dE_out=row[1])
        assert none is None and dE4.data_ptr() == row[1].data_ptr() and torch.equal(_bits(row[1]), _bits(dE)), name   # dL_drendered = NULL: the same dL_dE
        assert torch.isnan(row[0]).all() and torch.isnan(row[2]).all(), name                 # ... and 12 floats written, no more
        assert torch.equal(_bits(g), _bits(_t(c["g"]))) and torch.equal(_bits(img), _bits(_t(c["image"]))), name      # inputs untouched
    # E as a row of a (V, 12) tensor (4-byte aligned is enough) and as a host array
    c = cases[4]
    img, g = _t(c["image"]), _t(c["g"])
    rows = torch.zeros(25, device=_dev())[1:].view(2, 12)
    rows[1].copy_(_t(c["E"]))
    assert rows[1].data_ptr() % 16 == 4
    ref = X.apply_exposure(img, _t(c["E"]))
    assert torch.equal(_bits(X.apply_exposure(img, rows[1])), _bits(ref)) and torch.equal(_bits(X.apply_exposure(c["image"], c["E"])), _bits(ref))
    assert torch.equal(_bits(X.exposure_backward(img, rows[1], g)[1]), _bits(X.exposure_backward(c["image"], c["E"].reshape(4, 3), c["g"])[1]))
    return worst


def measure_adam():
    """The worst ratio of E, m, v against adam_run_f64 after 1, 2 and 1 000 steps of the fixed gradient sequence, on row 1 of a
    three-view model whose other rows must not move."""
    X = sub("exposure")
    worst = 0.0
    for T in (1, 2, 1000):
        grads = R.adam_gradients(T)
        E64, m64, v64, lrs = R.adam_run_f64(grads)
        model = X.ExposureModel(3, _dev())
        gd = _t(grads)
        for t in range(T):
            model.step(1, gd[t], lrs[t])
        assert model.steps == [0, T, 0]
        ident = _t(X.IDENTITY)
        for r in (0, 2):
            assert torch.equal(model.E[r], ident) and not model.m[r].any() and not model.v[r].any()
        gmax = float(np.abs(grads.astype(np.float64)).max())
        ratios = (np.abs(model.E[1].cpu().numpy() - E64) / (np.abs(E64) + sum(lrs)), np.abs(model.m[1].cpu().numpy() - m64) / gmax,
                  np.abs(model.v[1].cpu().numpy() - v64) / gmax ** 2)
        w = max(float(r.max()) for r in ratios) / EPS
        print(f"adam, {T} steps: worst ratio {w:.3f}; E moved by up to {np.abs(E64 - R.IDENTITY).max():.3e}")
        assert np.abs(E64 - R.IDENTITY).max() > 0.5 * lrs[0]                                 # a real step
        worst = max(worst, w)
    return worst


def _assert_margins(worst):
    m = _margins()
    for k, w in worst.items():
        assert m[k]["worst"] > 0 and abs(m[k]["K"] - 10.0 * m[k]["worst"]) <= 1e-9 * m[k]["K"], k
        assert w <= m[k]["K"], f"{k}: worst ratio {w:.3f} above K = {m[k]['K']:.3f} (measured {m[k]['worst']:.3f})"


def test_image_kernels_against_the_yardstick(cases):
    worst = measure_kernels(cases)
    print("\nworst error ratios (units of eps32 x error model):", json.dumps(worst))
    _assert_margins(worst)


def test_adam_against_the_yardstick():
    worst = {"adam": measure_adam()}
    print("\nworst error ratio (units of eps32 x error model):", json.dumps(worst))
    _assert_margins(worst)


def test_state_dict_round_trips_through_json():
    X = sub("exposure")
    model = X.ExposureModel(3, _dev())
    g = _t(R.adam_gradients(4))
    for t in range(4):
        model.step(t % 2, g[t], 0.01)
    state = json.loads(json.dumps(model.state_dict()))
    other = X.ExposureModel(3, _dev())
    other.load_state_dict(state)
    assert other.steps == model.steps == [2, 2, 0]
    for k in ("E", "m", "v"):
        assert torch.equal(_bits(getattr(other, k)), _bits(getattr(model, k))), k            # float32 -> JSON -> float32: the same bits
    model.step(0, g[0], 0.01), other.step(0, g[0], 0.01)
    assert torch.equal(_bits(other.E), _bits(model.E))                                       # ... and the same next step
    with pytest.raises(ValueError, match="state is not that of 2 views"):
        X.ExposureModel(2, _dev()).load_state_dict(state)


def test_composition_against_float64_and_identity_is_a_no_op(scenes, cameras):
    """render -> apply -> l1_loss_and_gradients -> exposure_backward on the toy scene at 64 x 64: dL_dE against the float64 autograd of
    the image-space graph L(E) = mean |img @ A + b - target|, and with E = identity the pixel gradient of the plain step, bit for bit."""
    gsr, X = pkg(), sub("exposure")
    from conftest import lego_camera
    sc = scenes.synthetic_scene(500, 0.05, 0.6, 3)
    kw = render_kwargs(sc, lego_camera(cameras, 0, 64, 64))
    img = gsr.render_gaussians(**kw)[0].reshape(64, 64, 3)
    img_np = img.cpu().numpy()
    assert (img_np > 0.05).mean() > 0.2
    rng = np.random.default_rng(8)
    E = (R.IDENTITY + rng.normal(0, 0.1, 12)).astype(np.float32)
    out64, _ = R.apply_f64(img_np, E)
    target = (out64 + rng.choice([-1.0, 1.0], out64.shape) * rng.uniform(0.05, 0.3, out64.shape)).astype(np.float32)   # no near-ties of the sign
    E_t, tg = _t(E), _t(target)
    img1 = X.apply_exposure(img, E_t)
    loss, dpix1 = gsr.loss.l1_loss_and_gradients(img1, tg)
    dpix, dE = X.exposure_backward(img, E_t, dpix1, out=dpix1)
    assert dpix is dpix1
    c = torch.tensor(img_np.astype(np.float64))
    E64 = torch.tensor(E.astype(np.float64).reshape(4, 3), requires_grad=True)
    L = (c @ E64[:3] + E64[3] - torch.tensor(target.astype(np.float64))).abs().mean()
    L.backward()
    g64 = np.sign(out64 - target.astype(np.float64)) / out64.size
    _, dE_closed, mag_img, mag_E = R.backward_closed(img_np, E, g64)
    assert np.allclose(E64.grad.numpy().reshape(12), dE_closed, rtol=1e-10, atol=0)
    K = _margins()["backward_E"]["K"] + 1.0                                                  # + the float32 rounding of the weight 1 / (3 W H)
    ratio = np.abs(dE.cpu().numpy() - E64.grad.numpy().reshape(12)) / mag_E / EPS
    print(f"\ncomposition: dL_dE worst ratio {ratio.max():.3f} (bound {K:.3f}); loss {float(loss.item()) / out64.size:.5f} against {float(L.detach()):.5f}")
    assert (ratio <= K).all()
    assert abs(float(loss.item()) / out64.size - float(L.detach())) <= 1e-5 * float(L.detach())
    # identity: the step without exposure, bit for bit
    _, plain = gsr.loss.l1_loss_and_gradients(img, tg)
    same = X.apply_exposure(img, _t(X.IDENTITY))
    assert torch.equal(_bits(same), _bits(img))
    _, d1 = gsr.loss.l1_loss_and_gradients(same, tg)
    d0, dE0 = X.exposure_backward(img, _t(X.IDENTITY), d1, out=d1)
    assert torch.equal(_bits(d0), _bits(plain))
    assert dE0.abs().max() > 0


def test_exposure_recovery_with_frozen_gaussians(scenes, cameras):
    """One view of a small synthetic scene at 48 x 40, target = image @ A* + b* (no clamp), 300 steps of ExposureModel.step on L1 alone,
    learning rate 0.01 -> 0.001: final L1 <= initial / 20 and max|E - E*| <= 2e-3.  tests/test_exposure_reference.py holds the float64
    yardstick to the same condition on the same case (there: x617 and 1.8e-4)."""
    gsr, X = pkg(), sub("exposure")
    q = R.RECOVERY
    _, _, kw, E_star = R.recovery_case(scenes, cameras, X.random_exposures)
    img = gsr.render_gaussians(**kw)[0].reshape(q["H"], q["W"], 3)
    target = _t(R.apply_f64(img.cpu().numpy(), E_star)[0])
    model = X.ExposureModel(2, _dev())
    curve = torch.zeros(q["steps"] + 1, device=_dev())
    n = float(img.numel())
    for t in range(q["steps"] + 1):
        out = X.apply_exposure(img, model.matrix(1))
        _, dpix = gsr.loss.l1_loss_and_gradients(out, target, loss_out=curve[t:t + 1])
        if t == q["steps"]:
            break
        _, dE = X.exposure_backward(img, model.matrix(1), dpix, want_image_grad=False)
        model.step(1, dE, R.decayed_lr(q["lr0"], q["lr1"], t, q["steps"]))
    curve = curve.cpu().numpy() / n
    err = float(np.abs(model.E[1].cpu().numpy().astype(np.float64) - E_star).max())
    ref = R.recover_f64(img.cpu().numpy(), E_star, q["steps"], q["lr0"], q["lr1"])
    print(f"\nrecovery: L1 {curve[0]:.3e} -> {curve[-1]:.3e} (x{curve[0] / curve[-1]:.1f}), max|E - E*| = {err:.3e}; "
          f"float64 on this image: x{ref['initial'] / ref['final']:.1f}, {ref['max_err']:.3e}")
    assert model.steps == [0, q["steps"]] and torch.equal(model.E[0], _t(X.IDENTITY))
    assert curve[-1] <= curve[0] / q["loss_factor"]
    assert err <= q["max_err"]


# ------------------------------------------------------------------------------------------- the trainer on Lego
def trainer_run(tmp, label, noise, seed, optimize):
    """One run of examples/train.py on the eight Lego views, 300 iterations: {"final_loss" (mean of the last 50 lines of the loss
    curve), "psnr" (mean training PSNR against the -- perturbed -- targets), "summary", "output"}."""
    log, out = os.path.join(tmp, f"{label}.jsonl"), os.path.join(tmp, label)
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train.py"), "--dataset", os.path.join(ROOT, "data", "lego"), "--views", "8", "--size", "100",
           "--iterations", "300", "--exposure-noise", str(noise), "--exposure-seed", str(seed), "--print-interval", "100", "--log", log,
           "--output", out, "--save-interval", "299"] + (["--optimize-exposure"] if optimize else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    recs = [json.loads(l) for l in open(log)]
    summary = [r for r in recs if r["record"] == "summary"][0]
    curve = np.concatenate([np.asarray(r["l1"], np.float64) for r in recs if r["record"] == "loss"])
    assert len(curve) == 300 and all(summary["parameters_finite"].values())
    return {"final_loss": float(curve[-50:].mean()), "psnr": float(summary["train_psnr_mean"]), "it_s": summary["iterations_per_s"], "summary": summary,
            "output": out}


def test_trainer_on_lego_recovers_from_exposure_noise(tmp_path):
    X = sub("exposure")
    m = _margins()["trainer"]
    plain = trainer_run(str(tmp_path), "plain", 0.2, 0, False)
    expo = trainer_run(str(tmp_path), "exposure", 0.2, 0, True)
    loss_gap, psnr_gap = plain["final_loss"] - expo["final_loss"], expo["psnr"] - plain["psnr"]
    print(f"\n--exposure-noise 0.2: final loss {plain['final_loss']:.5f} -> {expo['final_loss']:.5f} (gap {loss_gap:.5f}, required "
          f"{m['required_loss_gap']:.5f}); training PSNR {plain['psnr']:.2f} -> {expo['psnr']:.2f} dB (gap {psnr_gap:.2f}, required {m['required_psnr_gap']:.2f})")
    assert abs(m["required_loss_gap"] - 0.5 * min(m["loss_gaps"])) <= 1e-12 and abs(m["required_psnr_gap"] - 0.5 * min(m["psnr_gaps"])) <= 1e-12
    assert m["required_loss_gap"] > 0 and m["required_psnr_gap"] > 0
    assert loss_gap >= m["required_loss_gap"]
    assert psnr_gap >= m["required_psnr_gap"]
    s = expo["summary"]
    assert "exposure_final" not in plain["summary"]
    assert s["exposure_applied"] == {"train_views": True, "train_eval_scales": True, "holdout_views": False, "holdout_eval_scales": False}
    E = np.asarray(s["exposure_final"])
    assert E.shape == (8, 12) and np.isfinite(E).all() and sum(s["exposure_steps"]) == 300
    assert (np.abs(E - np.asarray(X.IDENTITY)).max(1) > 1e-3).all()                          # every view's matrix moved
    path = os.path.join(expo["output"], "point_cloud", "iteration_299", "exposure.json")
    with open(path) as fh:
        state = json.load(fh)
    model = X.ExposureModel(8, _dev())
    model.load_state_dict(state)                                                             # exposure.json reloads
    assert np.array_equal(model.E.cpu().numpy(), E.astype(np.float32)) and model.steps == s["exposure_steps"]
    assert os.path.exists(os.path.join(expo["output"], "point_cloud", "iteration_299", "point_cloud.ply"))


def test_trainer_exposure_does_not_hurt_clean_data(tmp_path):
    """--optimize-exposure at --exposure-noise 0 against the plain run: within the spread the plain noisy run showed from seed to seed."""
    m = _margins()["trainer"]
    plain = trainer_run(str(tmp_path), "clean_plain", 0.0, 0, False)
    expo = trainer_run(str(tmp_path), "clean_exposure", 0.0, 0, True)
    print(f"\nclean data: final loss {plain['final_loss']:.5f} / {expo['final_loss']:.5f} with exposure (allowed +{m['plain_loss_spread']:.5f}); "
          f"training PSNR {plain['psnr']:.2f} / {expo['psnr']:.2f} dB (allowed -{m['plain_psnr_spread']:.2f})")
    assert abs(m["plain_loss_spread"] - (max(m["plain_final_loss"]) - min(m["plain_final_loss"]))) <= 1e-12
    assert abs(m["plain_psnr_spread"] - (max(m["plain_psnr"]) - min(m["plain_psnr"]))) <= 1e-12
    assert expo["final_loss"] <= plain["final_loss"] + m["plain_loss_spread"]
    assert expo["psnr"] >= plain["psnr"] - m["plain_psnr_spread"]
