"""The normals stage on the MI355X (include/gsr_normals.h) against its float64 yardstick (tests/normals_reference.py: numpy and torch
autograd on the CPU, never the kernel itself).

Bounds.  `valid` is compared exactly: it is a float32 decision that the yardstick restates operation by operation.  Every other
output is held to K eps32 x (error model), with `worst` = the largest ratio measured on the MI355X over the case matrix
(normals_reference.all_cases) and K = 10 x worst, both in tests/golden/normals_margins.json beside the same ratios of a numpy float32
restatement of the formulas.  The error models, kappa the case's cancellation factor (normals_reference.kappa):
    normals   max |n - ref|                      / (eps32 kappa)
    gD, gA    max |g - ref| / max |ref|          / (eps32 kappa)
    sums      |s - ref| / |ref|                  / eps32
The file is written when it is absent (the first run on the device, trainer runs included) and asserted against when it is present.
measure_kernels() is the one place that forms the ratios and asserts the exact properties; every figure is printed before it is held.

The trainer's weight: --lambda-normal 0.05, the weight 2DGS gives its normal-consistency term; chosen once, not tuned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, lego_camera, pkg, render_kwargs, sub
import normals_reference as R

pytestmark = pytest.mark.gpu
EPS = R.EPS32
MARGINS = os.path.join(ROOT, "tests", "golden", "normals_margins.json")
LAMBDA_NORMAL = "0.05"
SEEDS = (0, 1, 2)           # --normal-seed of the three recorded trainer pairs
NORMAL_NOISE = "0.2"        # --normal-noise of the trainer runs: a prior about 11 degrees off per pixel
PARAM_GRADS = ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity")
SPREAD_FLOOR = 8e-4         # the aux-gradient bound of tests/test_gpu_aux_grads.py: float-atomic reordering of the backward, of max|g|
_margins_cache = {}


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(_dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def make_cases():
    """The case matrix with each case's float64 reference: computed once, shared by the tests, left unchanged."""
    _lib = sub("_lib")
    out = R.all_cases(_lib.NORMALS_TILE_W, _lib.NORMALS_TILE_H, _lib.NORMALS_MAX_BLOCKS)
    for c in out:
        c["ref"] = R.reference(c)
        c["kappa"] = R.kappa(c)
    return out


@pytest.fixture(scope="module")
def cases():
    return make_cases()


def _loss_call(c, **kw):
    args = dict(mask=_t(c["mask"]), weight=c["weight"], target_rotation=c["R"])
    args.update(kw)
    return sub("loss").normal_loss_and_gradients(_t(c["Dinv"]), _t(c["final_T"]), _t(c["target"]), c["cam"], **args)


def _direction32(c):
    """dL/dn of the fused loss as the header states it in float32, from numpy: -(weight m) t^ at the pixels that count, 0 elsewhere."""
    return R.loss_direction(c, np.float32)[0]


def measure_kernels(cases):
    """{"normals", "gD", "gA", "sums"}: the worst error ratio of each output on the matrix, every exact property asserted on every case."""
    N = sub("normals")
    worst = {"normals": 0.0, "gD": 0.0, "gA": 0.0, "sums": 0.0}
    side = torch.cuda.Stream(device=_dev())
    for c in cases:
        name, cam, ref = c["name"], c["cam"], c["ref"]
        D, T = _t(c["Dinv"]), _t(c["final_T"])
        n, valid = N.normals_from_depth(D, T, cam)
        sums, gD, gA = _loss_call(c)
        assert n.shape == (c["H"], c["W"], 3) and valid.shape == (c["H"], c["W"]) and sums.shape == (2,) and gD.shape == gA.shape == valid.shape, name
        for t in (n, valid, sums, gD, gA):
            assert bool(torch.isfinite(t).all()), name
        assert np.array_equal(valid.cpu().numpy() > 0, ref["valid"]), name                   # exactly the yardstick's decisions
        assert set(np.unique(valid.cpu().numpy())) <= {0.0, 1.0}, name
        assert not bool(_bits(n)[valid == 0].any()), name                                    # +0 where there is no normal
        if c["finite_only"]:
            print(f"{name:22s} finite ({int(ref['valid'].sum())} valid pixels)")
        else:
            got = {"normals": n.cpu().numpy(), "gD": gD.cpu().numpy(), "gA": gA.cpu().numpy(), "sums": sums.tolist()}
            e = R.error_ratios(got, ref, c["kappa"])
            print(f"{name:22s} kappa {c['kappa']:7.1f} sums {got['sums']}  errors: normals {e['normals']:.3f} gD {e['gD']:.3f} gA {e['gA']:.3f} "
                  f"(eps32 kappa) sums {e['sums']:.3f} (eps32)")
            for k in worst:
                worst[k] = max(worst[k], e[k])
        if c["degenerate"]:                                                                  # exactly zero, sums (0, 0)
            assert not bool(_bits(n).any()) and not bool(_bits(gD).any()) and not bool(_bits(gA).any()) and sums.tolist() == [0.0, 0.0], name
        else:
            assert bool(gD.any()) and bool(gA.any()), name
        undefined = torch.as_tensor(~c["dec"]["defined"]).to(_dev())
        assert not bool(_bits(gD)[undefined].any()) and not bool(_bits(gA)[undefined].any()), name    # +0 where the pixel is not defined
        # two calls: identical bits; then a workspace full of NaN; then a side stream
        again = _loss_call(c)
        assert all(_same(a, b) for a, b in zip(again, (sums, gD, gA))), name
        for (kind, _, _), ws in sub("_host")._ws.items():
            if kind == "normals":
                ws.fill_(0xFF)
        again = _loss_call(c)
        assert all(_same(a, b) for a, b in zip(again, (sums, gD, gA))), name
        side.wait_stream(torch.cuda.current_stream(_dev()))
        with torch.cuda.stream(side):
            again = _loss_call(c)
            n2, v2 = N.normals_from_depth(D, T, cam)
        side.synchronize()
        assert all(_same(a, b) for a, b in zip(again, (sums, gD, gA))) and _same(n2, n) and _same(v2, valid), name
        # want_grad=False: the same sums into the given slot and nothing else; R=None is the identity; mask=None a mask of ones
        slot = torch.full((3, 2), float("nan"), device=_dev())
        s3, none_D, none_A = _loss_call(c, want_grad=False, loss_out=slot[1])
        assert none_D is None and none_A is None and s3.data_ptr() == slot[1].data_ptr() and _same(slot[1], sums), name
        assert bool(torch.isnan(slot[0]).all()) and bool(torch.isnan(slot[2]).all()), name
        if c["R"] is None:
            assert all(_same(a, b) for a, b in zip(_loss_call(c, target_rotation=np.eye(3)), (sums, gD, gA))), name
        if c["mask"] is None:
            assert all(_same(a, b) for a, b in zip(_loss_call(c, mask=torch.ones_like(D)), (sums, gD, gA))), name
        # the fused loss shares the gather with the VJP: the VJP of the loss's own direction gives its bits
        g = _t(_direction32(c))
        vD, vA = N.normals_from_depth_backward(g, D, T, cam)
        assert _same(vD, gD) and _same(vA, gA), name
        # ... and torch.autograd through depth_to_normals gives the VJP's bits (final_Ts = 1 - alpha: negated)
        Dq, Tq = D.clone().requires_grad_(True), T.clone().requires_grad_(True)
        out = N.depth_to_normals(Dq, Tq, cam)
        assert _same(out, n), name
        aD, aT = torch.autograd.grad(out, (Dq, Tq), grad_outputs=g)
        assert _same(aD, vD) and _same(-aT, vA), name
        # inputs untouched
        assert _same(D, _t(c["Dinv"])) and _same(T, _t(c["final_T"])), name
    # an arbitrary dL/dn through the VJP, against autograd in float64 (the larger cases stand for the rest)
    rng = np.random.default_rng(17)
    for c in cases:
        if c["degenerate"] or c["finite_only"] or c["W"] * c["H"] > 1 << 14:
            continue
        g = rng.normal(0, 1, (c["H"], c["W"], 3)).astype(np.float32)
        vD, vA = N.normals_from_depth_backward(_t(g), _t(c["Dinv"]), _t(c["final_T"]), c["cam"])
        _, rD, rA = R.autograd_vjp(c, g)
        e = R.error_ratios({"normals": c["ref"]["normals"], "gD": vD.cpu().numpy(), "gA": vA.cpu().numpy(), "sums": ()},
                           {"normals": c["ref"]["normals"], "gD": rD, "gA": rA, "sums": ()}, c["kappa"])
        print(f"{c['name']:22s} VJP of a random dL/dn: gD {e['gD']:.3f} gA {e['gA']:.3f} (eps32 kappa)")
        worst["gD"], worst["gA"] = max(worst["gD"], e["gD"]), max(worst["gA"], e["gA"])
    return worst


def measure_restatement(cases):
    """The same ratios of the numpy float32 restatement (CPU)."""
    worst = {"normals": 0.0, "gD": 0.0, "gA": 0.0, "sums": 0.0}
    for c in cases:
        if c["degenerate"] or c["finite_only"]:
            continue
        e = R.error_ratios(R.restatement32(c), c["ref"], c["kappa"])
        for k in worst:
            worst[k] = max(worst[k], e[k])
    return worst


# ------------------------------------------------------------------------------------------------------- the ray convention
def ray_ratio(scenes, cameras):
    """Render 200 Gaussians at 64 x 48; for every visible one depths * ray(points_xy_image) against its camera-space mean in float64.
    Returns the worst |P - mean| / |mean| in eps32 and the number of visible Gaussians."""
    gsr = pkg()
    W, H = 64, 48
    sc = gsr.scenes.synthetic_scene(200, 0.05, 0.6, 5)
    cam = lego_camera(cameras, 0, W, H)
    _, _, buf = gsr.render_gaussians(**render_kwargs(sc, cam))
    vis = (buf["radii"].reshape(-1) > 0).cpu().numpy()
    xy = buf["points_xy_image"].cpu().numpy().astype(np.float64)[vis]
    z = buf["depths"].reshape(-1).cpu().numpy().astype(np.float64)[vis]
    rays = sub("normals").pixel_rays(cam)
    tx, ty = float(cam["tan_fovx"]), float(cam["tan_fovy"])
    ray = lambda px, py: np.stack([((2 * px + 1) / W - 1) * tx, ((2 * py + 1) / H - 1) * ty, np.ones_like(px)], -1)
    gx, gy = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    assert np.array_equal(ray(gx, gy), rays)                                               # pixel_rays is this formula at the integer pixels
    P = z[:, None] * ray(xy[:, 0], xy[:, 1])
    means = np.asarray(sc["means"], np.float64).reshape(-1, 3)[vis]
    cam_mean = (np.concatenate([means, np.ones((len(means), 1))], 1) @ np.asarray(cam["world_to_camera"], np.float64))[:, :3]
    err = np.linalg.norm(P - cam_mean, axis=1) / np.linalg.norm(cam_mean, axis=1)
    half = z[:, None] * ray(xy[:, 0] + 0.5, xy[:, 1] + 0.5)
    print(f"\nray convention: {int(vis.sum())} visible Gaussians, worst |depth ray - mean| / |mean| = {err.max():.3e} = {err.max() / EPS:.2f} eps32; "
          f"half a pixel off would give {(np.linalg.norm(half - cam_mean, axis=1) / np.linalg.norm(cam_mean, axis=1)).max():.1e}")
    return float(err.max() / EPS), int(vis.sum())


# ------------------------------------------------------------------------------------------------------- the trainer
def trainer_run(tmp, label, seed, *extra):
    """One run of examples/train.py in hidden-scene mode at 100 x 100, 300 iterations: its summary."""
    log = os.path.join(tmp, f"{label}.jsonl")
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train.py"), "--size", "100", "--views", "8", "--iterations", "300", "--normal-noise", NORMAL_NOISE,
           "--normal-seed", str(seed), "--print-interval", "1000", "--log", log, *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    summary = [r for r in map(json.loads, open(log)) if r["record"] == "summary"][0]
    assert all(summary["parameters_finite"].values())
    for k in ("train_normal_angle_deg_mean", "train_normal_valid_share", "train_psnr_mean"):
        assert summary[k] is not None and np.isfinite(summary[k]), k
    return summary


def trainer_pair(tmp, seed):
    """(with, without): the summaries of a run with the normal term on targets perturbed under `seed`, and of the run without it."""
    return (trainer_run(tmp, f"normal_{seed}", seed, "--lambda-normal", LAMBDA_NORMAL), trainer_run(tmp, f"plain_{seed}", seed))


def _margins(cases=None, scenes=None, cameras=None, tmp=None):
    """The margins file: read when present, measured and written when absent."""
    if "m" in _margins_cache:
        return _margins_cache["m"]
    if os.path.exists(MARGINS):
        with open(MARGINS) as fh:
            _margins_cache["m"] = json.load(fh)
        return _margins_cache["m"]
    worst, rest = measure_kernels(cases or make_cases()), measure_restatement(cases or make_cases())
    m = {k: {"worst": v, "K": 10.0 * v} for k, v in worst.items()}
    m["restatement32"] = rest
    ray, n_vis = ray_ratio(sub("scenes"), sub("cameras"))
    m["rays"] = {"worst": ray, "K": 10.0 * ray, "visible": n_vis}
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        pairs = [trainer_pair(d, s) for s in SEEDS]
    gaps = [b["train_normal_angle_deg_mean"] - a["train_normal_angle_deg_mean"] for a, b in pairs]
    holds = min(gaps) > 0
    m["trainer"] = {"lambda_normal": float(LAMBDA_NORMAL), "normal_noise": float(NORMAL_NOISE), "seeds": list(SEEDS),
                    "angle_with": [a["train_normal_angle_deg_mean"] for a, _ in pairs], "angle_without": [b["train_normal_angle_deg_mean"] for _, b in pairs],
                    "valid_share_with": [a["train_normal_valid_share"] for a, _ in pairs], "psnr_with": [a["train_psnr_mean"] for a, _ in pairs],
                    "psnr_without": [b["train_psnr_mean"] for _, b in pairs], "gaps": gaps, "claim_holds": holds,
                    "required_gap": 0.5 * min(gaps) if holds else None}
    with open(MARGINS, "w") as fh:
        json.dump(m, fh, indent=1)
        fh.write("\n")
    _margins_cache["m"] = m
    return m


def test_kernels_against_the_yardstick(cases):
    print()
    m = _margins(cases)
    worst = measure_kernels(cases)
    print("worst error ratios:", json.dumps(worst), " float32 numpy restatement:", json.dumps(m["restatement32"]))
    for k, w in worst.items():
        assert m[k]["worst"] > 0 and abs(m[k]["K"] - 10.0 * m[k]["worst"]) <= 1e-9 * m[k]["K"], k
        assert w <= m[k]["K"], f"{k}: worst ratio {w:.3f} above K = {m[k]['K']:.3f} (measured {m[k]['worst']:.3f})"


def test_ray_convention_matches_the_forward(cases, scenes, cameras):
    m = _margins(cases)["rays"]
    worst, n_vis = ray_ratio(scenes, cameras)
    assert n_vis >= 50
    assert m["worst"] > 0 and abs(m["K"] - 10.0 * m["worst"]) <= 1e-9 * m["K"]
    assert m["K"] * EPS < 1e-3                                                             # far below the 1e-2 of half a pixel
    assert worst <= m["K"], f"rays: {worst:.2f} eps32 above K = {m['K']:.2f}"


def test_loss_images_drive_the_backward_as_the_yardsticks_do(scenes, cameras):
    """The loss on a real render; both images into backward(); the parameter gradients against those from the float64 yardstick's
    images rounded to float32, within the aux-gradient bound (the backward's float atomics)."""
    gsr = pkg()
    W, H = 128, 96
    sc = gsr.scenes.synthetic_scene(3000, 0.05, 0.6, 7)
    cam = lego_camera(cameras, 0, W, H)
    kw = render_kwargs(sc, cam)
    _, dep, buf = gsr.render_gaussians(**kw)
    dep, Ts = dep.reshape(H, W), buf["final_Ts"].reshape(H, W)
    alpha_min = 0.2
    n, valid = gsr.normals.normals_from_depth(dep, Ts, cam, alpha_min)
    assert int(valid.sum().item()) >= 500
    rng = np.random.default_rng(9)
    target = (n.cpu().numpy() + 0.5 * rng.normal(0, 1, (H, W, 3))).astype(np.float32)
    c = {"Dinv": dep.cpu().numpy(), "final_T": Ts.cpu().numpy(), "cam": cam, "target": target, "R": None, "mask": None,
         "weight32": float(np.float32(0.3 / (W * H))), "dec": R.decide(dep.cpu().numpy(), Ts.cpu().numpy(), cam, alpha_min)}
    assert np.array_equal(valid.cpu().numpy() > 0, c["dec"]["valid"])
    ref = R.reference(c)
    sums, gD, gA = gsr.loss.normal_loss_and_gradients(dep, Ts, target, cam, weight=0.3, alpha_min=alpha_min)
    vD, vA = gsr.normals.normals_from_depth_backward(_t(R.loss_direction(c, np.float32)[0]), dep, Ts, cam, alpha_min)
    assert _same(vD, gD) and _same(vA, gA)
    e = R.error_ratios({"normals": n.cpu().numpy(), "gD": gD.cpu().numpy(), "gA": gA.cpu().numpy(), "sums": sums.tolist()}, ref, R.kappa(c))
    print(f"\nreal render: {int(valid.sum().item())} valid pixels, kappa {R.kappa(c):.1f}, sums {sums.tolist()}, errors {json.dumps(e)}")
    sets = []
    for dD, dA in ((gD, gA), (_t(ref["gD"]), _t(ref["gA"]))):
        b = backward_kwargs(sc, cam, kw, buf, None)
        b["geom_buffer"] = dict(b["geom_buffer"], depths=buf["depths"])
        g = gsr.backward(**b, dL_ddepth_image=dD, dL_dalpha_image=dA)
        sets.append({k: g[k].detach().cpu().numpy().astype(np.float64) for k in PARAM_GRADS})
    for k in PARAM_GRADS:
        assert np.isfinite(sets[0][k]).all() and np.abs(sets[0][k]).max() > 0, k
        moved = np.abs(sets[0][k] - sets[1][k]).max() / np.abs(sets[1][k]).max()
        print(f"{k}: kernel images against the yardstick's: {moved:.2e} of max|g| (bound {SPREAD_FLOOR:.0e})")
        assert moved <= SPREAD_FLOOR, k


def test_trainer_runs_with_the_normal_term(cases, tmp_path):
    """--iterations 300 --size 100, with --lambda-normal and without: both end finite and carry the summary fields.  The gap in the
    mean normal angle is required only if all three recorded pairs show one (tests/golden/normals_margins.json, "trainer"); then
    half the smallest recorded gap."""
    m = _margins(cases)["trainer"]
    with_n, without = trainer_pair(str(tmp_path), SEEDS[0])
    gap = without["train_normal_angle_deg_mean"] - with_n["train_normal_angle_deg_mean"]
    print(f"\nmean normal angle: {with_n['train_normal_angle_deg_mean']:.3f} deg with --lambda-normal {LAMBDA_NORMAL}, {without['train_normal_angle_deg_mean']:.3f} "
          f"without (gap {gap:.3f}; recorded gaps {m['gaps']}); valid share {with_n['train_normal_valid_share']:.3f} / {without['train_normal_valid_share']:.3f}; "
          f"PSNR {with_n['train_psnr_mean']:.2f} / {without['train_psnr_mean']:.2f} dB")
    assert len(m["gaps"]) == 3 and m["claim_holds"] == (min(m["gaps"]) > 0)
    if m["claim_holds"]:
        assert abs(m["required_gap"] - 0.5 * min(m["gaps"])) <= 1e-12 and gap >= m["required_gap"]
    else:
        assert m["required_gap"] is None
