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
5. The depth-distortion and depth-normal consistency terms.  Test 1 carries both (a synthetic normal image with pixels below the
   1e-3 length threshold and exactly zero; counted pixels within LENGTH_NEAR of the threshold aside).  On the training scene with
   the float64 forward's brute-force lists, classic and antialiased + filtered: blend_scalar_grads -- Dist by its moments, the
   normals as colours -- is autograd of the scalar written from the definitions (Dist as the double sum over pairs), in all six
   leaves, and the normals' gradient reaches dL_drot as autograd of n(q) and nothing else; camera_gradient_f64 is autograd of the
   whole chain camera -> geometry -> blend -> scalar in one (view, proj, campos) with the normals detached.  (param_half's geometry
   stage is f64_reference's VJP in the reference's convention, which is not the gradient of the forward -- its Q2 / Q3 -- so the
   identity is held stage by stage, not for the per-Gaussian chain as a whole.)  Every new mis-statement is load-bearing, as in 3.
   Each term is material: max|g_term| >= 0.1 max|g_total| for positions, scales and opacities (and rotations for the consistency
   term) on every view of the frames S7-S11 see.  The trainer's documented weights, --lambda-dist 100 and
   --lambda-normal-consistency 0.05, gave consistency shares of 0.02-0.18 (S8 0.05-0.16, S9 0.025-0.18, S11 0.035-0.10), so that
   weight is 0.5; with (100, 0.5) the smallest shares are S7 dist 0.34, S8 consistency 0.47, S9 dist 0.20 / consistency 0.26, S11
   dist 0.19 / consistency 0.36.  S10's frames follow the opacity reset (opacities <= 0.01): no pixel has alpha >= 0.5, 0.1 or 0.05,
   at --normal-alpha-min 0.02 61 pixels count and at 0.01 421, so S10 passes 0.01; Dist is O(alpha^2) there and its share at
   weight 100 was 0.005, at 1e4 0.05, so S10 alone passes --lambda-dist 1e5 (shares: dist 0.28, consistency 0.31).
6. What the camera gradient's contract leaves out: camera_gradient_full_f64 - camera_gradient_f64 with the consistency term's
   cotangents alone is 260 to 1250 x CAMERA_TRIP x sum|term| over the four views and both modes, so the GPU test does tell the
   contract from the full derivative, and normals_move_with_the_camera is a mis-statement.
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
    cfg = {"lam": 0.2, "window": "gaussian", "lam_d": 0.5, "depth_loss": depth_loss, "lam_a": 0.1, "lam_n": 0.05, "alpha_min": 0.5,
           "lam_dist": 100.0, "lam_nc": 0.5}
    # the normal image: unit-ish vectors, some shorter than the 1e-3 length threshold, some exactly (0, 0, 0)
    nimg = rng.normal(0, 1, (H, W, 3))
    nimg *= (rng.uniform(0.3, 1.0, (H, W)) / np.linalg.norm(nimg, axis=2))[..., None]
    u = rng.uniform(0, 1, (H, W))
    nimg[u < 0.06] *= 5e-4
    nimg[u < 0.03] = 0.0
    return {"img": img, "dinv": dinv, "final_T": fT, "cam": cam, "nimg": nimg.astype(np.float32)}, tg, cfg


@pytest.mark.parametrize("W,H", [(17, 13), (44, 44)])
@pytest.mark.parametrize("depth_loss", ["l1", "pearson"])
@pytest.mark.parametrize("weighted", [True, False])
def test_image_half_is_the_gradient_of_one_scalar(W, H, depth_loss, weighted):
    frame, tg, cfg = synthetic_view(W, H, 3 + W, depth_loss)
    if not weighted:
        tg = dict(tg, weights=None)
    res = S.image_half(frame, tg, cfg)
    assert res["kappa_n"] > 0 and np.abs(res["terms"]["normal_gD"]).max() > 0          # the normal term is alive
    assert res["counted"].sum() > 0.5 * W * H and (~res["counted"]).sum() > 0.03 * W * H and np.abs(res["terms"]["consistency_gA"]).max() > 0
    assert (np.asarray(frame["nimg"]) == 0).all(-1).any()
    leaves = [torch.tensor(np.asarray(frame[k], np.float64), requires_grad=True) for k in ("img", "dinv", "final_T")]
    dist, nimg = torch.zeros(H, W, dtype=torch.float64, requires_grad=True), torch.tensor(np.asarray(frame["nimg"], np.float64), requires_grad=True)
    g_img, g_d, g_T, g_dist, g_N = torch.autograd.grad(S.objective(*leaves, frame, tg, cfg, dist=dist, nimg=nimg), leaves + [dist, nimg])
    np.testing.assert_allclose(res["g_dist"], g_dist.numpy(), rtol=1e-8)
    far = ~res["near"]                                                                 # (counted is a float32 decision near the threshold)
    assert far.mean() > 0.99
    np.testing.assert_allclose(res["gN"][far], g_N.numpy()[far], rtol=1e-8, atol=1e-10 * np.abs(g_N.numpy()).max(), err_msg="gN")
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
    mine = set(S.IMAGE_MISS) | set(S.STEP_MISS) | set(S.PARAM_MISS) | set(S.TERM_IMAGE_MISS) | set(S.TERM_PARAM_MISS) | set(S.CAMERA_MISS)
    assert mine == set(S.MISSTATEMENTS)


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


# ---- 5. the distortion and consistency terms ----
# The weights and the --normal-alpha-min of S10 that tests/test_gpu_train_step.py passes: settled by
# test_each_regulariser_is_material_on_the_frames_the_gpu_configurations_see below (module docstring).
LAMBDA_DIST, LAMBDA_NC = 100.0, 0.5
S10_LAMBDA_DIST, S10_ALPHA_MIN = 1e5, 0.01
TERM_CONFIGS = {
    # name: (rasterize mode, filtered, parameters as after the opacity reset, cfg)
    "S7": ("classic", False, False, {"lam": 0.2, "lam_dist": LAMBDA_DIST}),
    "S8": ("classic", False, False, {"lam_nc": LAMBDA_NC, "lam_n": 0.05, "lam_d": 0.5, "lam_a": 0.1}),
    "S9": ("antialiased", True, False, {"lam_dist": LAMBDA_DIST, "lam_nc": LAMBDA_NC}),
    "S10": ("classic", False, True, {"lam_dist": S10_LAMBDA_DIST, "lam_nc": LAMBDA_NC, "dist_from_iter": 1, "nc_from_iter": 1, "it": 1,
                                     "alpha_min": S10_ALPHA_MIN}),
    "S11": ("classic", False, False, {"lam": 0.2, "lam_dist": LAMBDA_DIST, "lam_nc": LAMBDA_NC}),
}


@functools.lru_cache(maxsize=None)
def term_frame(v, mode, filtered, reset):
    """View v of the training scene by the float64 forward on brute-force lists, as the image half takes a frame (float32 images),
    with the float64 normals and their image, and targets rendered from the hidden scene the same way."""
    cams, hidden, P = train_scene()
    if reset:                                                                        # iteration 0 ends with the opacity reset
        P = dict(P, opacities=np.minimum(P["opacities"], np.float32(0.01)))
    f3d = S.FR.sampling_f64(P["positions"], cams, 0.2)["filter_3d"].astype(np.float32) if filtered else None
    pre = S.preprocess(P, cams[v], mode, f3d)
    pl, ranges = S.brute_force_lists(pre)
    img, dinv, fT, _ = S.forward_f64(pre, pl, ranges, mode)
    normals, _ = S.gaussian_normals_f64(P, cams[v])
    dist, nimg = S.regulariser_images_f64(pre, pl, ranges, mode, normals)
    Ph = {"positions": hidden["means"], "scales": hidden["scales"], "rotations": hidden["rotations"], "opacities": hidden["opacities"], "shs": hidden["shs"]}
    pre_h = S.preprocess(Ph, cams[v], mode)
    h_img, h_dinv, h_T, _ = S.forward_f64(pre_h, *S.brute_force_lists(pre_h), mode)
    rng = np.random.default_rng(5 + v)
    f32 = lambda a: np.asarray(a, np.float32)
    tg = {"target": f32(h_img), "weights": None, "E": None, "depth_target": f32(h_dinv), "depth_mask": (h_dinv > 0).astype(np.float32),
          "alpha_target": f32(1.0 - h_T), "normal_target": rng.normal(0, 1, (SIZE, SIZE, 3)).astype(np.float32), "normal_rot": None}
    frame = {"img": f32(img), "dinv": f32(dinv), "final_T": f32(fT), "nimg": f32(nimg), "dist": dist, "cam": cams[v]}
    return {"P": P, "cam": cams[v], "f3d": f3d, "pre": pre, "pl": pl, "ranges": ranges, "normals": normals, "frame": frame, "tg": tg, "mode": mode}


def term_gradients(f, cfg, only=None, miss=None):
    """param_half of a term_frame under cfg.  only: None (every term), "dist" or "nc" (that term's cotangents alone)."""
    half = S.image_half(f["frame"], f["tg"], dict({"window": "gaussian", "alpha_min": 0.5}, **cfg), miss=miss)
    cot = {"dpix": half["dpix"], "gD": half["gD"], "gA": half["gA"], "g_dist": half["g_dist"], "gN": half["gN"]}
    if only == "dist":
        cot = {"dpix": None, "gD": None, "gA": None, "g_dist": half["g_dist"], "gN": None}
    elif only == "nc":
        t = half["terms"]
        cot = {"dpix": None, "gD": t["consistency_gD"], "gA": t["consistency_gA"], "g_dist": None, "gN": half["gN"]}
    return S.param_half(f["P"], f["cam"], f["pl"], f["ranges"], cot["dpix"], cot["gD"], cot["gA"], rasterize_mode=f["mode"], filter_3d=f["f3d"],
                        pre=f["pre"], g_dist=cot["g_dist"], gN=cot["gN"], normals=f["normals"], miss=miss), half


def test_each_regulariser_is_material_on_the_frames_the_gpu_configurations_see():
    """max|g_term| >= 0.1 max|g_total| for positions, scales and opacities (and rotations for the consistency term), on every view
    of every configuration: below that the colour gradient hides a wrong term inside parity.assert_grad's bands."""
    shares = {}
    for name, (mode, filtered, reset, cfg) in TERM_CONFIGS.items():
        for v in range(VIEWS):
            f = term_frame(v, mode, filtered, reset)
            total, half = term_gradients(f, cfg)
            for term, lam, groups in (("dist", "lam_dist", ("positions", "scales", "opacities")),
                                      ("nc", "lam_nc", ("positions", "scales", "opacities", "rotations"))):
                if cfg.get(lam, 0.0) <= 0.0:
                    continue
                alone, _ = term_gradients(f, cfg, only=term)
                if term == "nc":
                    assert half["counted"].sum() >= 50 and np.abs(half["terms"]["consistency_gD"]).max() > 0, (name, v, int(half["counted"].sum()))
                for k in groups:
                    g = S.GROUP_OF[k]
                    share = float(np.abs(alone[g]).max() / np.abs(total[g]).max())
                    key = f"{name}/{term}/{k}"
                    shares[key] = min(shares.get(key, np.inf), share)
    print("\nsmallest share max|g_term| / max|g_total| over the views: " + ", ".join(f"{k} {v:.2f}" for k, v in shares.items()))
    low = {k: v for k, v in shares.items() if v < 0.1}
    assert not low, low


def _weights(f, leaves, idx, xt, yt):
    """(w (P, L), final T (P,)) of one tile: the blend's weights handed out by the mode's tile function, one colour channel per entry."""
    tile = S.AR._blend_tile if f["mode"] == "antialiased" else S.F._blend_tile
    xy, con, op, col, invd = leaves
    L = idx.numel()
    onehot = torch.zeros(xy.shape[0], L, dtype=torch.float64)
    onehot[idx, torch.arange(L)] = 1.0
    out, _, T, _ = tile(xy, con, op, onehot, invd, idx, xt, yt, torch.zeros(L, dtype=torch.float64), True)
    return out, T


def _scalar_by_definition(f, leaves, n, cots):
    """sum_p dpix . C + gD Dinv + gA (1 - T) + g Dist + gN . N written from the definitions: Dist as the double sum over pairs
    w_i w_j (m_i - m_j)^2, j < i (include/gsr_distortion.h), N as sum_k w_k n[i_k]."""
    dpix, gD, gA, g_dist, gN = (torch.as_tensor(np.asarray(c, np.float64)) for c in cots)
    xy, con, op, col, invd = leaves
    bg = f["pre"]["cam"].bg
    pl = torch.as_tensor(np.asarray(f["pl"], np.int64))
    total = torch.zeros((), dtype=torch.float64)
    for s, e, yy, xx in S.F._tiles(SIZE, SIZE, f["ranges"]):
        if e <= s:
            continue
        idx = pl[s:e]
        yt, xt = torch.as_tensor(yy), torch.as_tensor(xx)
        w, T = _weights(f, leaves, idx, xt.to(torch.float64), yt.to(torch.float64))
        m = invd[idx]
        pair = torch.tril((m[:, None] - m[None, :]) ** 2, diagonal=-1)                       # [i, j], j < i
        Dist = torch.einsum("pi,ij,pj->p", w, pair, w)
        total = (total + ((w @ col[idx] + T[:, None] * bg[None, :]) * dpix[yt, xt]).sum() + ((w @ m) * gD[yt, xt]).sum()
                 + ((1.0 - T) * gA[yt, xt]).sum() + (Dist * g_dist[yt, xt]).sum() + ((w @ n[idx]) * gN[yt, xt]).sum())
    return total


def _seeded_cotangents(seed=9):
    rng = np.random.default_rng(seed)
    px = SIZE * SIZE
    return (rng.normal(0, 1, (SIZE, SIZE, 3)) / (3 * px), rng.normal(0, 1, (SIZE, SIZE)) / px, rng.normal(0, 1, (SIZE, SIZE)) / px,
            rng.uniform(0.5, 1.5, (SIZE, SIZE)) * 100.0 / px, rng.uniform(-1, 1, (SIZE, SIZE, 3)) / px)


@pytest.mark.parametrize("mode,filtered", [("classic", False), ("antialiased", True)])
def test_blend_stage_with_the_two_terms_is_the_gradient_of_one_scalar(mode, filtered):
    """blend_scalar_grads (the moments form of Dist, the normals as colours) against autograd of the scalar written from the
    definitions, in all six leaves; and the normals' gradient carried to the rotations against autograd of n(q) itself.  The
    geometry stage behind the five blend leaves is f64_reference's VJP in the reference's convention, which is not the gradient of
    the forward (its Q2 / Q3) and stays held as before: by test 2 and tests/test_f64_reference.py."""
    f = term_frame(0, mode, filtered, False)
    pre, cots = f["pre"], _seeded_cotangents()
    depth = pre["depth"].detach()
    invd = torch.where(depth > 0, 1.0 / torch.where(depth > 0, depth, torch.ones_like(depth)), torch.zeros_like(depth))
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    leaves = [leaf(pre[k]) for k in ("xy", "conic", "opacity", "colour")] + [leaf(invd)]
    n = torch.tensor(f["normals"], requires_grad=True)
    ref = torch.autograd.grad(_scalar_by_definition(f, leaves, n, cots), leaves + [n])
    tile = S.AR._blend_tile if mode == "antialiased" else S.F._blend_tile
    got = S.blend_scalar_grads(tile, [leaf(t) for t in leaves], f["pl"], f["ranges"], SIZE, SIZE, pre["cam"].bg, True, *cots, normals=f["normals"])
    for name, g, r in zip(("xy", "conic", "opacity", "colour", "invd", "normals"), got, ref):
        assert r.abs().max() > 0, name
        np.testing.assert_allclose(g.numpy(), r.numpy(), rtol=1e-8, atol=1e-10 * float(r.abs().max()), err_msg=name)
    # normals -> rotations: c* and sigma held, the raw scales' axis
    P, cam = f["P"], f["cam"]
    q = torch.tensor(np.asarray(P["rotations"], np.float64), requires_grad=True)
    r = S.NRR.normals_f64(P["scales"], P["rotations"], P["positions"], cam["world_to_camera"], q_tensor=q)
    g_n = got[5].numpy()
    (dq,) = torch.autograd.grad((r["n_t"] * torch.as_tensor(g_n)).sum(), q)
    np.testing.assert_allclose(S.normals_to_rotations_f64(P, cam, f["normals"], g_n), dq.numpy(), rtol=1e-8, atol=1e-12 * float(dq.abs().max()))
    # ... and param_half adds exactly that to dL_drot, nothing to the other groups
    with_n = S.param_half(P, cam, f["pl"], f["ranges"], None, rasterize_mode=mode, filter_3d=f["f3d"], pre=pre, gN=cots[4], normals=f["normals"])
    no_rot = S.param_half(P, cam, f["pl"], f["ranges"], None, rasterize_mode=mode, filter_3d=f["f3d"], pre=pre, gN=cots[4], normals=f["normals"],
                          miss=["consistency_rot_dropped"])
    np.testing.assert_allclose(with_n["dL_drot"] - no_rot["dL_drot"], dq.numpy(), rtol=1e-8, atol=1e-10 * float(dq.abs().max()))
    for k in ("dL_dmean3D", "dL_dscale", "dL_dopacity", "dL_dshs"):
        assert np.array_equal(with_n[k], no_rot[k]), k


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_camera_gradient_with_the_two_terms_is_autograd_in_the_camera_leaves(mode):
    """camera_gradient_f64 (two stages, per-Gaussian leaves) against autograd of the whole chain camera -> geometry -> blend ->
    scalar in ONE (view, proj, campos), the normals detached: the library's contract."""
    f = term_frame(1, mode, False, False)
    P, cots, aa = f["P"], _seeded_cotangents(4), mode == "antialiased"
    sc, kw = S.scene_of(P), S.render_kw(f["cam"])
    radii = f["pre"]["radii"]
    grad, scale = S.camera_gradient_f64(sc, kw, radii, f["pl"], f["ranges"], *cots[:3], antialiased=aa, g_dist=cots[3], gN=cots[4], normals=f["normals"])
    cam = S.CR.Cam(kw)
    sub, idx, N = S.CR._visible(sc, radii)
    V, Pm, C = (t.clone().requires_grad_(True) for t in (cam.view, cam.proj, cam.campos))
    xy, con, col, invd = S.CR._scatter(N, idx, *S.CR.geometry(sub, kw, cam, V, Pm, C, 3, 1.0))
    op = S.F._t(sub["opacities"], (int(idx.numel()),))
    if aa:
        op = op * S.AR._rho_of_camera(sub, kw, cam, V.expand(int(idx.numel()), 4, 4), 1.0)
    op = S.CR._scatter(N, idx, op)[0]
    L = _scalar_by_definition(f, [xy, con, op, col, invd], torch.as_tensor(f["normals"]), cots)
    ref = torch.cat([g.reshape(-1) for g in torch.autograd.grad(L, (V, Pm, C))]).numpy()
    assert (scale[:35] >= np.abs(grad[:35]) * (1 - 1e-9)).all() and np.abs(ref).max() > 0
    err = np.abs(grad[:35] - ref) / (1e-8 * np.abs(ref) + 1e-9 * scale[:35] + 1e-300)      # (sum |term| is what a sum of 600 terms rounds against)
    assert err.max() <= 1.0, (err.max(), grad[:35], ref)
    # each term reaches the camera, and the classic mode without them is still camera_grad_reference's
    for k in (3, 4):
        part = S.camera_gradient_f64(sc, kw, radii, f["pl"], f["ranges"], antialiased=aa, g_dist=cots[3] if k == 3 else None,
                                     gN=cots[4] if k == 4 else None, normals=f["normals"])[0]
        assert np.abs(part).max() > 1e-3 * np.abs(grad).max(), k
    if not aa:
        g0, s0 = S.camera_gradient_f64(sc, kw, radii, f["pl"], f["ranges"], *cots[:3])
        g1, s1 = S.CR.camera_gradient_f64(sc, kw, radii, f["pl"], f["ranges"], *cots[:3])
        np.testing.assert_allclose(g0, g1, rtol=1e-10, atol=1e-14 * np.abs(g1).max())
        np.testing.assert_allclose(s0, s1, rtol=1e-10)


ALL_TERMS = {"lam": 0.2, "lam_d": 0.5, "lam_a": 0.1, "lam_n": 0.05, "lam_dist": LAMBDA_DIST, "lam_nc": LAMBDA_NC, "window": "gaussian", "alpha_min": 0.5}


@pytest.mark.parametrize("name", S.TERM_IMAGE_MISS)
def test_regulariser_image_misstatement_is_load_bearing(name):
    """On view 0 with every term on: the flip moves one of the five cotangent images by more than 10 x image_half_bounds; an image
    that is held exactly (dL_ddistortion), or that appears or vanishes, counts as moved by any difference at all."""
    f = term_frame(0, "classic", False, False)
    cfg = dict(ALL_TERMS, dist_from_iter=1, nc_from_iter=1, it=0) if name == "from_iter_ignored" else ALL_TERMS
    ref, bad = S.image_half(f["frame"], f["tg"], cfg), S.image_half(f["frame"], f["tg"], cfg, miss=[name])
    bounds = S.image_half_bounds(ref, f["tg"], cfg)
    ratios = {}
    for k in ("dpix", "gD", "gA", "g_dist", "gN"):
        a, b = ref[k], bad[k]
        if a is None and b is None:
            continue
        d = float(np.abs((0.0 if a is None else a) - (0.0 if b is None else b)).max())
        ratios[k] = d / bounds[k] if bounds[k] > 0 else (np.inf if d > 0 else 0.0)
    print(f"\n{name}: moves the outputs by {({k: f'{v:.3g}' for k, v in ratios.items()})} x their bounds")
    assert max(ratios.values()) > 10.0, ratios


@pytest.mark.parametrize("mode,filtered", [("classic", False), ("antialiased", True)])
@pytest.mark.parametrize("name", S.TERM_PARAM_MISS + S.TERM_IMAGE_MISS[:5])
def test_regulariser_misstatement_moves_the_gradients(name, mode, filtered):
    """... and every one of them, the image ones handed on as wrong cotangents, leaves parity.assert_grad's bands by 10 x in a group."""
    f = term_frame(0, mode, filtered, False)
    cfg = {k: v for k, v in ALL_TERMS.items() if k != "lam"}
    ref, _ = term_gradients(f, cfg)
    bad, _ = term_gradients(f, cfg, miss=[name])
    hit = [k for k in S.SMALL if moved(ref[S.GROUP_OF[k]], bad[S.GROUP_OF[k]])]
    print(f"\n{name} ({mode}): moves {hit}")
    assert hit, name
    if name == "consistency_rot_dropped":
        assert hit == ["rotations"]


# ---- 6. what the camera gradient's contract leaves out ----
CAMERA_TRIP = 8.9e-4         # tests/test_gpu_camera_grads.py TRIP (tests/test_gpu_train_step.py asserts the copies equal their owner)


def omitted_camera_term(v, mode):
    """max over the 35 camera floats of |camera_gradient_full_f64 - camera_gradient_f64| / (CAMERA_TRIP sum|term|), the consistency
    term's cotangents alone (gN with its own gD and gA)."""
    f = term_frame(v, mode, False, False)
    half = S.image_half(f["frame"], f["tg"], {"lam_nc": LAMBDA_NC, "alpha_min": 0.5})
    sc, kw = S.scene_of(f["P"]), S.render_kw(f["cam"])
    args = (sc, kw, f["pre"]["radii"], f["pl"], f["ranges"], None, half["gD"], half["gA"])
    kwargs = dict(antialiased=mode == "antialiased", gN=half["gN"], normals=f["normals"])
    g, s = S.camera_gradient_f64(*args, **kwargs)
    g_full, _ = S.camera_gradient_full_f64(*args, **kwargs)
    g_miss, _ = S.camera_gradient_f64(*args, **kwargs, miss=S.CAMERA_MISS)
    assert np.array_equal(g_miss, g_full)
    live = s[:35] > 0
    return float((np.abs(g_full - g)[:35][live] / (CAMERA_TRIP * s[:35][live])).max())


def test_the_camera_term_the_contract_leaves_out_is_measured():
    """The normals' direct dependence on viewmatrix is deliberately not in the library's camera gradient
    (include/gsr_normal_render.h (b)).  Measured here, in units of the bound the GPU test applies (module docstring): above 10 the
    GPU test tells the contract from the full derivative, and MISSTATEMENTS says so."""
    figures = {f"{mode}/view{v}": omitted_camera_term(v, mode) for mode in ("classic", "antialiased") for v in range(VIEWS)}
    print("\nomitted camera term / (CAMERA_TRIP sum|term|): " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))
    assert min(figures.values()) > 0
    assert ("normals_move_with_the_camera" in S.MISSTATEMENTS) == (min(figures.values()) > 10.0), figures
