"""
tests/step_reference.py, the float64 statement of one training step, checked on the CPU.  No GPU.

1. Image half against autograd: torch float64 autograd of L_v as ONE scalar (step_reference.objective) reproduces the composed
   (dpix, gD, gA) of step_reference.image_half, on synthetic 17 x 13 and 44 x 44 images with every term on (masked L1 or Pearson
   depth), a non-identity exposure matrix and a weight image.  final_T holds multiples of 2^-12, so the float32 1 - T of the
   statement is the exact one autograd differentiates.
2. Classic mode against the oracle: on the scene, cameras and size tests/test_gpu_train_step.py trains (600 Gaussians, seed 8,
   four orbit cameras at 44 x 44, targets rendered from the hidden seed-7 scene), the oracle's float32 per-view gradients of the
   L1 pixel gradient, averaged over a batch, meet parity.assert_grad against the float64 batch mean, view by view and for the
   four-view batch; the SH group also rebuilt from the views' payloads, which must agree with the dense one.  This is the evidence
   that a correct float32 evaluation passes on these inputs.  Lists come from the oracle's forward.  The antialiased, auxiliary
   and filtered modes have no float32 CPU restatement (the oracle renders the classic mode alone): for them the float64 statement
   is held to its own parts instead (test 3 moves it, tests/test_antialias_reference.py and tests/test_filter3d_reference.py hold the parts).
3. Every entry of MISSTATEMENTS is load-bearing: flipping it moves at least one output by more than 10 x the bound the GPU test
   applies to that output -- step_reference.image_half_bounds for the three images, parity.assert_grad's bands for the gradients.
   Classic-mode entries run on the oracle's lists; those that need the antialiased mode or the filter on the float64 forward's own
   (preprocess_f64's radii and rectangles, brute-force tile lists).
4. The camera gradient under the antialiased mode with the auxiliary images reduces to antialias_reference's colour-only one and is
   linear in the three images; the central-difference chain to xi is pose.pose_gradient's autograd.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import backward_kwargs, render_kwargs, sub
import parity
import step_reference as S

SIZE, N, VIEWS = 44, 600, 4


@functools.lru_cache(maxsize=None)
def train_scene():
    """What examples/train.py --size 44 --gaussians 600 --views 4 --init random starts from: (cams, hidden scene, parameters)."""
    scenes, cameras = sub("scenes"), sub("cameras")
    cams = [cameras.nerf_camera(scenes.orbit_pose(k, VIEWS), SIZE, SIZE, scenes.LEGO_CAMERA_ANGLE_X) for k in range(VIEWS)]
    hidden, init = scenes.synthetic_scene(N, 0.05, 0.5, seed=7), scenes.synthetic_scene(N, 0.05, 0.5, seed=8)
    P = {"positions": init["means"], "scales": init["scales"], "rotations": init["rotations"], "opacities": init["opacities"], "shs": init["shs"]}
    return cams, hidden, {k: np.ascontiguousarray(v, np.float32) for k, v in P.items()}


@functools.lru_cache(maxsize=None)
def oracle_frames():
    """Per view: the oracle's classic forward of the parameters, the target (its render of the hidden scene), the L1 pixel gradient
    and the oracle's float32 backward of it."""
    from oracle import oracle as o
    o.lib()
    cams, hidden, P = train_scene()
    sc = {"means": P["positions"], "scales": P["scales"], "rotations": P["rotations"], "opacities": P["opacities"], "shs": P["shs"]}
    out = []
    for cam in cams:
        kw = render_kwargs(sc, cam)
        target = np.asarray(o.render_gaussians(**render_kwargs(hidden, cam))[0], np.float32).reshape(SIZE, SIZE, 3)
        img, dep, buf = o.render_gaussians(**kw)
        frame = {"img": np.asarray(img).reshape(SIZE, SIZE, 3), "dinv": np.asarray(dep).reshape(SIZE, SIZE),
                 "final_T": np.asarray(buf["final_Ts"]).reshape(SIZE, SIZE), "cam": cam}
        half = S.image_half(frame, {"target": target}, {"lam": 0.0})
        dpix = half["dpix"].astype(np.float32)
        g = o.backward(**backward_kwargs(sc, cam, kw, buf, dpix))
        out.append({"cam": cam, "frame": frame, "target": target, "buf": buf, "dpix": dpix, "g": g, "half": half})
    return out


# ---- 1. image half against autograd ----
def synthetic_view(W, H, seed, depth_loss):
    rng = np.random.default_rng(seed)
    cam = {"tan_fovx": 0.4, "tan_fovy": 0.4 * H / W, "width": W, "height": H}
    xx, yy = np.meshgrid(np.arange(W) / W, np.arange(H) / H)
    z = 3.0 + 0.5 * np.sin(4.0 * xx + 0.5) * np.cos(3.0 * yy) + 0.3 * xx + 0.02 * rng.uniform(-1, 1, (H, W))
    fT = (rng.integers(1, 1200, (H, W)) / 4096.0).astype(np.float32)               # multiples of 2^-12 below 0.3: 1 - T is exact
    fT[rng.uniform(0, 1, (H, W)) < 0.03] = np.float32(0.75)                          # holes: alpha below alpha_min
    dinv = ((1.0 - fT.astype(np.float64)) / z).astype(np.float32)
    img = rng.uniform(0.05, 0.95, (H, W, 3)).astype(np.float32)
    E = (S.XR.IDENTITY + rng.normal(0, 0.1, 12)).astype(np.float32)
    target = rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    w = rng.uniform(0.2, 1.0, (H, W)).astype(np.float32)
    w[H // 3:H // 3 + 4, W // 4:W // 4 + 5] = 0.0
    dt = (0.7 * dinv + 0.05 + rng.normal(0, 0.03, (H, W))).astype(np.float32)
    dt[rng.uniform(0, 1, (H, W)) < 0.1] = 0.0
    tg = {"target": target, "weights": w, "E": E, "depth_target": dt, "depth_mask": (dt > 0).astype(np.float32),
          "alpha_target": rng.uniform(0, 1, (H, W)).astype(np.float32), "normal_target": rng.normal(0, 1, (H, W, 3)).astype(np.float32),
          "normal_rot": None}
    cfg = {"lam": 0.2, "window": "gaussian", "lam_d": 0.5, "depth_loss": depth_loss, "lam_a": 0.1, "lam_n": 0.05, "alpha_min": 0.5}
    return {"img": img, "dinv": dinv, "final_T": fT, "cam": cam}, tg, cfg


@pytest.mark.parametrize("W,H", [(17, 13), (44, 44)])
@pytest.mark.parametrize("depth_loss", ["l1", "pearson"])
@pytest.mark.parametrize("weighted", [True, False])
def test_image_half_is_the_gradient_of_one_scalar(W, H, depth_loss, weighted):
    frame, tg, cfg = synthetic_view(W, H, 3 + W, depth_loss)
    if not weighted:
        tg = dict(tg, weights=None)
    res = S.image_half(frame, tg, cfg)
    assert res["kappa_n"] > 0 and np.abs(res["terms"]["normal_gD"]).max() > 0          # the normal term is alive
    leaves = [torch.tensor(np.asarray(frame[k], np.float64), requires_grad=True) for k in ("img", "dinv", "final_T")]
    g_img, g_d, g_T = torch.autograd.grad(S.objective(*leaves, frame, tg, cfg), leaves)
    x = S.corrected(frame["img"], tg["E"])
    keep = (np.abs(x - tg["target"].astype(np.float64)) >= 1e-9).all(-1)
    assert keep.mean() > 0.99
    for name, got, ref in (("dpix", res["dpix"][keep], g_img.numpy()[keep]), ("gD", res["gD"], g_d.numpy()), ("gA", res["gA"], -g_T.numpy())):
        assert np.abs(ref).max() > 0, name
        np.testing.assert_allclose(got, ref, rtol=1e-8, atol=1e-10 * np.abs(ref).max(), err_msg=name)
    # dL/dE: the closed form against autograd of the same scalar in E
    E = torch.tensor(np.asarray(tg["E"], np.float64), requires_grad=True)
    img64 = torch.as_tensor(np.asarray(frame["img"], np.float64))
    xE = img64 @ E.reshape(4, 3)[:3] + E.reshape(4, 3)[3]
    y = torch.as_tensor(np.asarray(tg["target"], np.float64))
    L = S.WR.loss(xE, y, torch.as_tensor(np.asarray(tg["weights"], np.float64)), cfg["lam"]) if weighted else S.DS.loss(xE, y, cfg["lam"])
    np.testing.assert_allclose(res["dE"], torch.autograd.grad(L, E)[0].numpy(), rtol=1e-8, atol=1e-12)


# ---- 2. classic mode against the oracle ----
def _views64(idx, **kw):
    cams, _, P = train_scene()
    fr = oracle_frames()
    return [S.param_half(P, fr[v]["cam"], fr[v]["buf"]["point_list"], fr[v]["buf"]["ranges"], fr[v]["dpix"], **kw) for v in idx]


@functools.lru_cache(maxsize=None)
def _all_views64():
    return _views64(range(VIEWS))


def test_tie_pixels_stay_inside_the_cap_on_the_oracle_frames():
    for f in oracle_frames():
        share = S.tie_pixels(f["frame"]["img"], None, f["target"]).mean()
        assert share <= 1e-3, share


def test_oracle_float32_composite_meets_the_float64_composite():
    cams, _, P = train_scene()
    fr, v64 = oracle_frames(), _all_views64()
    for v in range(VIEWS):                                                           # the float64 side was given the oracle's lists: same visibility
        pre = S.preprocess(P, cams[v])
        assert np.array_equal(np.asarray(fr[v]["buf"]["radii"]) > 0, ~pre["culled"])
    worst = {}
    for batch in ([0], [1], [2], [3], [0, 1, 2, 3]):
        G64 = S.step_gradient([v64[v] for v in batch], len(batch), P["positions"])
        G64p = S.step_gradient([v64[v] for v in batch], len(batch), P["positions"], sh="payloads")
        # the two statements of the SH gradient agree (the payload rows pass through float32 in adam_reference: 6e-8 of a row)
        np.testing.assert_allclose(G64p["shs"], G64["shs"], rtol=0, atol=2e-7 * np.abs(G64["shs"]).max())
        for k, name in S.GROUP_OF.items():
            g32 = sum(np.asarray(fr[v]["g"][name], np.float32).reshape(G64[k].shape) for v in batch) * np.float32(1.0 / len(batch))
            assert np.abs(G64[k]).max() > 0, k
            ok, rel = parity.assert_grad(f"batch {batch} {k}", g32, G64[k])
            worst[k] = max(worst.get(k, 0.0), rel)
    print("\noracle composite vs float64, worst max err / max|g|:", {k: f"{v:.2e}" for k, v in worst.items()})


# ---- 3. every mis-statement is load-bearing ----
def moved(ref, flipped):
    """True when `flipped` lies more than 10 x outside what parity.assert_grad allows around `ref`: the largest difference above
    10 x the loose band, or 10 x as many elements as may leave the tight band outside 10 x that band."""
    ref, flipped = np.asarray(ref, np.float64), np.asarray(flipped, np.float64)
    m = np.abs(ref).max()
    err = np.abs(flipped - ref)
    allowed = max(1.0 - 0.999, 4.0 / ref.size)
    return bool(err.max() > 10.0 * parity.GRAD_REST * m) or bool((err > 10.0 * (parity.GRAD_ABS * m + parity.GRAD_REL * np.abs(ref))).mean() > 10.0 * allowed)


@functools.lru_cache(maxsize=None)
def s2_like_view():
    """View 0's oracle frame with every image term on: the S2 row's lambdas, a non-identity exposure and an occluder mask."""
    cams, hidden, P = train_scene()
    f = oracle_frames()[0]
    from oracle import oracle as o
    h_img, h_dep, h_buf = o.render_gaussians(**render_kwargs(hidden, cams[0]))
    hT = np.asarray(h_buf["final_Ts"]).reshape(SIZE, SIZE)
    rng = np.random.default_rng(5)
    w = np.ones((SIZE, SIZE), np.float32)
    w[10:22, 25:36] = 0.0
    dt = np.asarray(h_dep, np.float32).reshape(SIZE, SIZE)
    tg = {"target": f["target"], "weights": w, "E": (S.XR.IDENTITY + rng.normal(0, 0.1, 12)).astype(np.float32), "depth_target": dt,
          "depth_mask": (dt > 0).astype(np.float32), "alpha_target": (1.0 - hT).astype(np.float32),
          "normal_target": rng.normal(0, 1, (SIZE, SIZE, 3)).astype(np.float32), "normal_rot": None}
    cfg = {"lam": 0.2, "window": "gaussian", "lam_d": 0.5, "depth_loss": "l1", "lam_a": 0.1, "lam_n": 0.05, "alpha_min": 0.5}
    return f["frame"], tg, cfg


@pytest.mark.parametrize("name", S.IMAGE_MISS)
def test_image_misstatement_is_load_bearing(name):
    frame, tg, cfg = s2_like_view()
    ref, bad = S.image_half(frame, tg, cfg), S.image_half(frame, tg, cfg, miss=[name])
    bounds = S.image_half_bounds(ref, tg, cfg)
    ratios = {k: float(np.abs(bad[k] - ref[k]).max()) / bounds[k] for k in ("dpix", "gD", "gA")}
    print(f"\n{name}: moves the outputs by {({k: f'{v:.3g}' for k, v in ratios.items()})} x their bounds")
    assert max(ratios.values()) > 10.0, ratios


@pytest.mark.parametrize("name", S.STEP_MISS)
def test_batch_mean_misstatement_is_load_bearing(name):
    _, _, P = train_scene()
    v64 = _all_views64()[:2]
    for sh in ("dense", "payloads"):
        ref, bad = S.step_gradient(v64, 2, P["positions"], sh=sh), S.step_gradient(v64, 2, P["positions"], miss=[name], sh=sh)
        hit = [k for k in ref if moved(ref[k], bad[k])]
        assert hit == (["shs"] if name == "no_mean_sh" else list(S.SMALL)), (sh, hit)


@functools.lru_cache(maxsize=None)
def mode_case():
    """View 0 under the antialiased mode and the 3D filter, on the float64 forward's own lists, with seeded cotangent images."""
    cams, _, P = train_scene()
    f3d = S.FR.sampling_f64(P["positions"], cams, 0.2)["filter_3d"].astype(np.float32)
    assert (f3d > 0).all()
    pre = S.preprocess(P, cams[0], "antialiased", f3d)
    pl, ranges = S.brute_force_lists(pre)
    assert len(pl) > 1000
    rng = np.random.default_rng(9)
    cots = (rng.normal(0, 1, (SIZE, SIZE, 3)) / (3 * SIZE * SIZE), rng.normal(0, 1, (SIZE, SIZE)) / SIZE ** 2, rng.normal(0, 1, (SIZE, SIZE)) / SIZE ** 2)
    ref = S.param_half(P, cams[0], pl, ranges, *cots, rasterize_mode="antialiased", filter_3d=f3d, pre=pre)
    return P, cams[0], pl, ranges, cots, f3d, pre, ref


@pytest.mark.parametrize("name", S.PARAM_MISS)
def test_mode_misstatement_is_load_bearing(name):
    P, cam, pl, ranges, cots, f3d, pre, ref = mode_case()
    bad = S.param_half(P, cam, pl, ranges, *cots, rasterize_mode="antialiased", filter_3d=f3d, miss=[name], pre=pre)
    hit = [k for k in S.GROUP_OF.values() if moved(ref[k], bad[k])]
    print(f"\n{name}: moves {hit}")
    assert hit, name


def test_every_misstatement_has_a_check():
    assert set(S.IMAGE_MISS) | set(S.STEP_MISS) | set(S.PARAM_MISS) == set(S.MISSTATEMENTS)


def test_filtered_antialiased_statement_reduces_to_its_parts():
    """With a zero filter and the classic mode param_half is f64_reference.backward_f64 on the same lists (dpix alone), and the
    float64 forward of the stated modes is finite and differs from the classic one (the modes are live at this size)."""
    cams, _, P = train_scene()
    fr = oracle_frames()[0]
    sc = {"means": P["positions"], "scales": P["scales"], "rotations": P["rotations"], "opacities": P["opacities"], "shs": P["shs"]}
    r = S.F.backward_f64(sc, render_kwargs(sc, cams[0]), fr["buf"]["point_list"], fr["buf"]["ranges"], fr["dpix"])
    got = _all_views64()[0]
    for k in S.GROUP_OF.values():
        np.testing.assert_allclose(got[k], r[k], rtol=1e-9, atol=1e-13 * np.abs(r[k]).max(), err_msg=k)
    P2, cam, pl, ranges, cots, f3d, pre, ref = mode_case()
    img_aa = S.forward_f64(pre, pl, ranges, "antialiased")[0]
    pre_c = S.preprocess(P, cam)
    img_c = S.forward_f64(pre_c, *S.brute_force_lists(pre_c))[0]
    assert np.isfinite(img_aa).all() and np.abs(img_aa - img_c).max() > 1e-3


# ---- 4. the camera gradient under the modes, and its chain to xi ----
def test_antialiased_camera_gradient_extends_the_colour_only_one():
    """With the depth and alpha cotangents absent the extension is antialias_reference.camera_gradient_aa_f64; with them it is
    linear in the three images (the blend is, and so is every VJP behind it)."""
    P, cam, pl, ranges, cots, f3d, pre, _ = mode_case()
    sc, kw = S.scene_of(P), S.render_kw(cam)
    pre0 = S.preprocess(P, cam, "antialiased")
    pl0, r0 = S.brute_force_lists(pre0)
    radii = pre0["radii"]
    g, s = S.camera_gradient_f64(sc, kw, radii, pl0, r0, cots[0], antialiased=True)
    g_ref, s_ref = S.AR.camera_gradient_aa_f64(sc, kw, radii, pl0, r0, cots[0])
    np.testing.assert_allclose(g, g_ref, rtol=1e-10, atol=1e-14 * np.abs(g_ref).max())
    np.testing.assert_allclose(s, s_ref, rtol=1e-10)
    g_all = S.camera_gradient_f64(sc, kw, radii, pl0, r0, *cots, antialiased=True)[0]
    parts = sum(S.camera_gradient_f64(sc, kw, radii, pl0, r0, *[c if j == i else None for j, c in enumerate(cots)], antialiased=True)[0] for i in range(3))
    np.testing.assert_allclose(g_all, parts, rtol=1e-9, atol=1e-12 * np.abs(g_all).max())
    assert np.abs(g_all - g).max() > 1e-3 * np.abs(g).max()                          # the two auxiliary images do reach the camera


def test_pose_chain_by_central_differences_is_the_trainers_autograd():
    """pose_gradient_f64's chain to xi against pose.pose_gradient (autograd through the SE(3) exponential) of the same 35 floats."""
    pose = sub("pose")
    cams, _, P = train_scene()
    fr = oracle_frames()[1]
    rng = np.random.default_rng(2)
    start = pose.apply_pose_delta(cams[1], pose.random_pose_delta(rng, 1.0, 0.0))
    xi = rng.normal(0, 0.01, 6)
    cam = pose.apply_pose_delta(start, xi)
    pre = S.preprocess(P, cam)
    pl, ranges = S.brute_force_lists(pre)
    gD = rng.normal(0, 1, (SIZE, SIZE)) / SIZE ** 2
    dxi, reach = S.pose_gradient_f64(P, start, xi, pre["radii"], pl, ranges, fr["dpix"], gD, None, apply_pose_delta=pose.apply_pose_delta)
    g36 = S.camera_gradient_f64(S.scene_of(P), S.render_kw(cam), pre["radii"], pl, ranges, fr["dpix"], gD, None)[0]
    ref = pose.pose_gradient(start, xi, g36[:16].reshape(4, 4), g36[16:32].reshape(4, 4), g36[32:35])
    assert np.abs(ref).max() > 0 and (reach >= np.abs(dxi) * (1 - 1e-9)).all()
    np.testing.assert_allclose(dxi, ref, rtol=1e-6, atol=1e-8 * np.abs(ref).max())
