"""
tests/depth_step_reference.py, the float64 statement of the three --depth-render terms in a training step, checked on the CPU.  No GPU.

The scene is the one tests/test_gpu_depth_step.py trains -- 600 Gaussians (seed 8), four orbit cameras at 44 x 44, targets from the
hidden seed-7 scene -- after that file's prepare() hook, whose numbers are settled and exported here (prepared_params, MASK_HOLE): the
positions pulled towards the centre by POSITION_SHRINK = 0.45 (the model then leaves a border of the image empty: pixels without a
median), the scales flattened by plane_depth_reference.plane_scales and grown by SCALE_GAIN = 1.75 (at 2 the filter turns only about
twenty flat Gaussians round, at 1.5 one filtered view has a single clamped chosen entry, at 1 no view has two), the opacities multiplied by OPACITY_GAIN = 2.5
and held to OPACITY_CAP = 0.95 (transmittance falls through one half on a third of a view), and a 12 x 14 rectangle of
every depth mask cleared (the hidden scene covers every pixel: without it the target's mask decides nothing).  Frames are the float64
forward's on brute-force lists, as tests/test_step_reference.py has them; the contributor image is
median_depth_reference.median_f64's, the median and plane-median images are the float32 values its entries name, the plane image is
plane_depth_reference.render_f32's.

1. Each term is the gradient of one differentiable torch scalar written from the definitions, the contributor (and every clamp and
   branch) held fixed: sum_p g invd[id(p)] (median), sum_p g m_id(p)(p) over the unclamped pixels (plane-median),
   sum_p g sum_k w_k(p) m_k(p) (plane), with m_k(p) = invd_k + gx_k (p.x - x_k) + gy_k (p.y - y_k) from (positions, rotations) in
   float64.  Positions and rotations against term_gradients' moments half; under plane also the yardstick's blend columns against
   autograd in (xy, conic, opacity).  Tolerance: tests/test_step_reference.py's, rtol 1e-8.  (The geometry stage behind the blend
   columns is f64_reference's VJP in the reference's convention, held by tests/test_f64_reference.py, as there.)
2. Every entry of MISSTATEMENTS is visible: applied to the float64 side, on view MISS_VIEW (one every configuration draws at
   iteration 0), it moves the mode's cotangent image (or dL_ddepth_image) by more than 10 x image_half_bounds, or a gradient group
   out of parity.assert_grad's bands by 10 x (test_step_reference.moved).
3. The conditions the GPU test asserts hold for the reference alone on every view of every configuration D1-D8 (CONFIGS): ties, the
   share of pixels with a median, with a true crossing, where the mask's factors decide, free chosen entries, Gaussians flat raw and
   round filtered, and the term's share of sum |g| (>= 10 % for positions, and rotations where the term reaches them); clamped
   chosen entries on every view but the first orbit view (depth_step_reference.NO_CLAMP_VIEW says why).  FIRST_VIEWS names the views
   iteration 0 of each configuration draws; the GPU test asserts that the trainer drew them.
   --lambda-depth is LAMBDA_DEPTH = 12: at 2 the plane-median term's share of the rotations' sum |g| was 0.014-0.05 on views 1-3;
   at 12 the smallest shares are 0.12 (rotations, D6 / D7 view 3) and 0.49 (positions, D1 view 1).
"""
import functools

import numpy as np
import pytest
import torch

import depth_step_reference as DS
import median_depth_reference as M
import normal_render_reference as NRR
import plane_depth_reference as PD
import plane_median_reference as PM
import step_reference as S
from test_step_reference import LAMBDA_NC, SIZE, VIEWS, _weights, moved, train_scene

LAMBDA_DEPTH = 12.0
POSITION_SHRINK, SCALE_GAIN, OPACITY_GAIN, OPACITY_CAP = 0.45, 1.75, 2.5, 0.95
MISS_VIEW = 3                                        # the view the mis-statements are applied on: one every configuration draws at iteration 0
MASK_HOLE = (slice(12, 24), slice(16, 30))          # rows, columns of every view's depth mask that prepare() clears
MIN_FLAT_TO_ROUND = 10
MIN_SHARE = 0.10
# name: (mode, antialiased + filtered, the lambdas of the remaining terms) -- tests/test_gpu_depth_step.py's rows
CONFIGS = {
    "D1": ("median", False, {"lam_d": LAMBDA_DEPTH, "lam_n": 0.05, "lam_a": 0.1}),
    "D2": ("plane-median", False, {"lam_d": LAMBDA_DEPTH, "lam": 0.2}),
    "D3": ("plane", False, {"lam_d": LAMBDA_DEPTH, "lam_nc": LAMBDA_NC, "lam_n": 0.05}),
    "D4": ("plane", False, {"lam_nc": LAMBDA_NC}),
    "D5": ("plane-median", True, {"lam_d": LAMBDA_DEPTH}),
    "D6": ("plane-median", False, {"lam_d": LAMBDA_DEPTH}),
    "D7": ("plane-median", False, {"lam_d": LAMBDA_DEPTH}),
    "D8": ("median", False, {"lam_d": LAMBDA_DEPTH}),
}
# the views iteration 0 of each configuration draws (the trainer's seeded batch stream: numpy's default_rng(0))
FIRST_VIEWS = {"D1": (2, 3), "D2": (2, 3), "D3": (3,), "D4": (3,), "D5": (3,), "D6": (2, 3), "D7": (3, 2, 0, 1), "D8": (3,)}
f32 = np.float32


def prepared_params(P):
    """The prepare() hook's arithmetic on float32 arrays: flat Gaussians (most take the plane branch) and opacities high enough that
    transmittance falls through one half on part of the image."""
    P = dict(P)
    n = np.asarray(P["positions"]).reshape(-1, 3).shape[0]
    P["positions"] = (np.asarray(P["positions"], f32) * f32(POSITION_SHRINK)).astype(f32)
    P["scales"] = (PD.plane_scales(np.asarray(P["scales"], f32).reshape(n, 3)) * f32(SCALE_GAIN)).astype(f32)
    P["opacities"] = np.minimum(np.asarray(P["opacities"], f32) * f32(OPACITY_GAIN), f32(OPACITY_CAP)).astype(f32)
    return P


@functools.lru_cache(maxsize=None)
def depth_frame(v, mode, filtered):
    """View v of the prepared scene by the float64 forward on brute-force lists, with everything the two halves read."""
    cams, hidden, P0 = train_scene()
    P, cam = prepared_params(P0), cams[v]
    rmode = "antialiased" if filtered else "classic"
    f3d = S.FR.sampling_f64(P["positions"], cams, 0.2)["filter_3d"].astype(f32) if filtered else None
    pre = S.preprocess(P, cam, rmode, f3d)
    pl, ranges = S.brute_force_lists(pre)
    img, dinv, fT, nc = S.forward_f64(pre, pl, ranges, rmode)
    n = pre["N"]
    nb = {"points_xy_image": pre["xy"].detach().numpy().astype(f32), "point_list": pl, "ranges": ranges, "n_contrib": np.asarray(nc, np.int32),
          "conic_opacity": np.concatenate([pre["conic"].detach().numpy(), pre["opacity"].detach().numpy().reshape(n, 1)], 1).astype(f32),
          "depths": pre["depth"].detach().numpy().astype(f32)}
    fr = DS.frame_of(nb, SIZE, SIZE)
    ref = M.median_f64(fr)
    view = np.asarray(cam["world_to_camera"], f32).reshape(4, 4)
    n32 = NRR.normals_f32(P["scales"], P["rotations"], P["positions"], view)[0]
    normals, flipped = S.gaussian_normals_f64(P, cam, captured=n32)
    sl32, _ = PD.slopes_f32(n32, P["scales"], P["positions"], view, cam["tan_fovx"], cam["tan_fovy"], SIZE, SIZE)
    contrib = ref["contrib"]
    if mode == "median":
        depth_img = ref["med"]
    elif mode == "plane-median":
        depth_img = PM.chosen(fr, sl32, contrib)["m"]
    else:
        depth_img, contrib = PD.render_f32(fr, sl32)[0], None
    nimg = S.regulariser_images_f64(pre, pl, ranges, rmode, normals)[1]
    Ph = {"positions": hidden["means"], "scales": hidden["scales"], "rotations": hidden["rotations"], "opacities": hidden["opacities"], "shs": hidden["shs"]}
    pre_h = S.preprocess(Ph, cam, rmode)
    h_img, h_dinv, h_T, _ = S.forward_f64(pre_h, *S.brute_force_lists(pre_h), rmode)
    rng = np.random.default_rng(5 + v)
    mask = (h_dinv > 0).astype(f32)
    mask[MASK_HOLE] = 0
    tg = {"target": f32(h_img), "weights": None, "E": None, "depth_target": f32(h_dinv), "depth_mask": mask,
          "alpha_target": f32(1.0 - h_T), "normal_target": rng.normal(0, 1, (SIZE, SIZE, 3)).astype(f32), "normal_rot": None}
    frame = {"img": f32(img), "dinv": f32(dinv), "final_T": f32(fT), "nimg": f32(nimg), "cam": cam, "depth_img": depth_img, "contrib": contrib}
    return {"P": P, "cam": cam, "f3d": f3d, "pre": pre, "pl": pl, "ranges": ranges, "mode": rmode, "depth_mode": mode, "fr": fr, "nb": nb, "ref": ref,
            "normals": normals, "flipped": flipped, "n32": n32, "slopes": sl32, "frame": frame, "tg": tg}


def cfg_of(lams):
    return dict({"window": "gaussian", "alpha_min": 0.5, "depth_loss": "l1"}, **lams)


def halves(f, lams, miss=None):
    """(image half, the view's gradients) of a depth_frame under the lambdas."""
    mode, cfg = f["depth_mode"], cfg_of(lams)
    half = DS.image_half(mode, f["frame"], f["tg"], cfg, miss=miss)
    rest = S.param_half(f["P"], f["cam"], f["pl"], f["ranges"], half["dpix"], half["gD"], half["gA"], rasterize_mode=f["mode"], filter_3d=f["f3d"],
                        pre=f["pre"], gN=half["gN"], normals=f["normals"])
    term = DS.term_gradients(mode, f["P"], f["cam"], f["pre"], f["fr"], half["g_term"], f["frame"]["contrib"], f["slopes"], f["normals"],
                             filter_3d=f["f3d"], miss=miss, nb=f["nb"])
    return half, DS.view_gradients(rest, term)


def test_every_misstatement_has_a_check():
    assert set(DS.IMAGE_MISS) | set(DS.PARAM_MISS) | set(DS.STEP_MISS) == set(DS.MISSTATEMENTS) == set(DS.MODE_OF)


# ---- 1. each term is the gradient of one scalar ----
def _plane_of(f, p_t, q_t):
    """(invd, gx, gy, x, y) per Gaussian, float64 torch in the leaves (positions, rotations), from the definitions
    (include/gsr_plane_depth.h): the camera-space normal of the raw scales' shortest axis with its side held, t = n . p_v,
    gx = n_x kx / t, and (0, 0) where the captured slopes say the Gaussian fell back."""
    P, cam = f["P"], f["cam"]
    V = torch.tensor(np.asarray(cam["world_to_camera"], np.float64).reshape(4, 4))
    side = torch.as_tensor(np.where(f["flipped"], -1.0, 1.0))
    n = NRR.normals_f64(P["scales"], P["rotations"], P["positions"], cam["world_to_camera"], q_tensor=q_t)["n_t"] * side[:, None]
    pv = p_t @ V[:3, :3] + V[3, :3]
    front = pv[:, 2].detach() > 0
    z = torch.where(front, pv[:, 2], torch.ones_like(pv[:, 2]))
    invd = torch.where(front, 1.0 / z, torch.zeros_like(z))
    fb = torch.as_tensor(~(f["slopes"] != 0).any(1))
    t = torch.where(fb, torch.ones_like(z), (n * pv).sum(1))
    kx, ky = 2.0 * cam["tan_fovx"] / SIZE, 2.0 * cam["tan_fovy"] / SIZE
    zero = torch.zeros_like(z)
    gx, gy = torch.where(fb, zero, n[:, 0] * kx / t), torch.where(fb, zero, n[:, 1] * ky / t)
    x, y = PD.pixel_of(torch.stack([pv[:, 0], pv[:, 1], z], 1), cam["tan_fovx"], cam["tan_fovy"], SIZE, SIZE)
    return invd, gx, gy, x, y


def _leaves(f):
    return (torch.tensor(np.asarray(f["P"]["positions"], np.float64).reshape(-1, 3), requires_grad=True),
            torch.tensor(np.asarray(f["P"]["rotations"], np.float64).reshape(-1, 4), requires_grad=True))


def _close(name, got, ref):
    assert np.abs(ref).max() > 0, name
    np.testing.assert_allclose(got, ref, rtol=1e-8, atol=1e-10 * np.abs(ref).max(), err_msg=name)


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("mode", ["median", "plane-median"])
def test_chosen_entry_terms_are_the_gradient_of_one_scalar(mode, filtered):
    f = depth_frame(0, mode, filtered)
    g = PD.draw_g(SIZE, SIZE).astype(np.float64)
    p_t, q_t = _leaves(f)
    invd, gx, gy, x, y = _plane_of(f, p_t, q_t)
    # (the frame carries the exact float64 projections, as plane_median_reference allows: the moments then hold the very centres
    # the scalar is written in, and the identity is exact)
    fr = dict(f["fr"], xy=torch.stack([x, y], 1).detach().numpy())
    term = DS.term_gradients(mode, f["P"], f["cam"], f["pre"], fr, g, f["frame"]["contrib"], f["slopes"], f["normals"], filter_3d=f["f3d"])
    ch = PM.chosen(fr, f["slopes"], f["frame"]["contrib"])
    ids = torch.as_tensor(np.where(ch["ids"] >= 0, ch["ids"], 0))
    gt = torch.as_tensor(g)
    if mode == "median":
        L = (gt * invd[ids])[torch.as_tensor(ch["ids"] >= 0)].sum()
    else:
        ys, xs = torch.meshgrid(torch.arange(SIZE, dtype=S.D), torch.arange(SIZE, dtype=S.D), indexing="ij")
        m = invd[ids] + gx[ids] * (xs - x[ids]) + gy[ids] * (ys - y[ids])
        # the float64 m is the captured image's value at every unclamped pixel: the statement reads the same plane the kernel drew
        free = (ch["ids"] >= 0) & ~ch["clamped"]
        assert np.abs(m.detach().numpy() - ch["m"])[free].max() <= 1e-5 * np.abs(ch["m"]).max()
        L = (gt * m)[torch.as_tensor(free)].sum()
    dp, dq = torch.autograd.grad(L, (p_t, q_t), allow_unused=True)
    _close("positions", term["dL_dmean3D"], dp.numpy())
    if mode == "median":
        assert dq is None and not term["dL_drot"].any()
    else:
        _close("rotations", term["dL_drot"], dq.numpy())
    assert not term["dL_dscale"].any() and not term["dL_dopacity"].any()


def test_plane_term_is_the_gradient_of_one_scalar():
    f = depth_frame(0, "plane", False)
    g = PD.draw_g(SIZE, SIZE).astype(np.float64)
    term = DS.term_gradients("plane", f["P"], f["cam"], f["pre"], f["fr"], g, None, f["slopes"], f["normals"], nb=f["nb"])
    assert term["masked"] <= DS.MAX_MASKED
    assert np.array_equal(term["dL_dopacity"], term["yardstick"]["dL_dopacity"]["signed"][:, 0])
    pre = f["pre"]
    p_t, q_t = _leaves(f)
    invd, gx, gy, x, y = _plane_of(f, p_t, q_t)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    # the yardstick on the exact float64 arrays the scalar is written in (centres, slopes, inverse depths): the identity is then exact
    xy, con, op = leaf(torch.stack([x, y], 1)), leaf(pre["conic"]), leaf(pre["opacity"])
    nb = dict(f["nb"], points_xy_image=xy.detach().numpy(), conic_opacity=torch.cat([con, op[:, None]], 1).detach().numpy())
    r = PD.yardstick(nb, SIZE, SIZE, invd.detach().numpy(), torch.stack([gx, gy], 1).detach().numpy(), g)
    assert r["mask"].mean() <= DS.MAX_MASKED
    gt = torch.as_tensor(r["g"])                                        # (zero at the yardstick's masked pixels)
    pl = torch.as_tensor(np.asarray(f["pl"], np.int64))
    L = torch.zeros((), dtype=S.D)
    for s, e, yy, xx in S.F._tiles(SIZE, SIZE, f["ranges"]):
        if e <= s:
            continue
        idx = pl[s:e]
        yt, xt = torch.as_tensor(yy), torch.as_tensor(xx)
        w, _ = _weights(f, [xy, con, op, pre["colour"].detach(), invd.detach()], idx, xt.to(S.D), yt.to(S.D))
        mr = invd[idx][None, :] + gx[idx][None, :] * (xt.to(S.D)[:, None] - x[idx][None, :]) + gy[idx][None, :] * (yt.to(S.D)[:, None] - y[idx][None, :])
        lo, hi = 0.25 * invd[idx][None, :], 4.0 * invd[idx][None, :]
        m = torch.where(mr < lo, lo.detach().expand_as(mr), torch.where(mr > hi, hi.detach().expand_as(mr), mr))      # the clamp is held constant
        L = L + (gt[yt, xt] * (w * m).sum(1)).sum()
    dp, dq, dxy, dcon, dop = torch.autograd.grad(L, (p_t, q_t, xy, con, op))
    view_mean, view_rot, _ = DS._moments_to_parameters(f["P"], f["cam"], f["normals"], ~(f["slopes"] != 0).any(1), r["dL_dplane_moments"]["signed"])
    _close("positions", view_mean, dp.numpy())
    _close("rotations", view_rot, dq.numpy())
    # the blend columns, in the kernel's conventions (mean2D in NDC units, B as stored)
    _close("mean2D", r["dL_dmean2D"]["signed"], dxy.numpy() * np.array([0.5 * SIZE, 0.5 * SIZE]))
    _close("conic", r["dL_dconic"]["signed"][:, [0, 1, 3]], dcon.numpy() * np.array([1.0, 0.5, 1.0]))
    _close("opacity", r["dL_dopacity"]["signed"][:, 0], dop.numpy())
    assert np.abs(term["dL_dscale"]).max() > 0 and np.abs(term["dL_dopacity"]).max() > 0 and np.abs(term["dL_drot"]).max() > 0


# ---- 2. every mis-statement is visible ----
def _config_of(name):
    mode = DS.MODE_OF[name]
    if name == "filtered_scales_for_the_plane":
        return "D5"
    return {"median": "D1", "plane-median": "D2", "plane": "D3"}[mode]


@pytest.mark.parametrize("name", DS.IMAGE_MISS)
def test_image_misstatement_is_load_bearing(name):
    mode, filtered, lams = CONFIGS[_config_of(name)]
    f, cfg = depth_frame(MISS_VIEW, mode, filtered), cfg_of(lams)
    ref, bad = DS.image_half(mode, f["frame"], f["tg"], cfg), DS.image_half(mode, f["frame"], f["tg"], cfg, miss=[name])
    bounds = DS.image_half_bounds(mode, ref, f["tg"], cfg)
    ratios = {}
    for k in ("g_term", "gD", "gA"):
        a, b = ref[k], bad[k]
        if a is None and b is None:
            continue
        d = float(np.abs((0.0 if a is None else a) - (0.0 if b is None else b)).max())
        ratios[k] = d / bounds[k] if bounds[k] > 0 else (np.inf if d > 0 else 0.0)
    print(f"\n{name}: moves the images by {({k: f'{v:.3g}' for k, v in ratios.items()})} x their bounds")
    assert max(ratios.values()) > 10.0, ratios


@pytest.mark.parametrize("name", DS.PARAM_MISS)
def test_parameter_misstatement_is_load_bearing(name):
    mode, filtered, lams = CONFIGS[_config_of(name)]
    f = depth_frame(MISS_VIEW, mode, filtered)
    ref, bad = halves(f, lams)[1], halves(f, lams, miss=[name])[1]
    hit = [k for k in S.SMALL if moved(ref[S.GROUP_OF[k]], bad[S.GROUP_OF[k]])]
    print(f"\n{name}: moves {hit}")
    assert hit, name
    if name == "plane_median_rot_dropped":
        assert hit == ["rotations"]


def test_batch_mean_misstatement_is_load_bearing():
    mode, filtered, lams = CONFIGS["D2"]
    views = [halves(depth_frame(v, mode, filtered), lams)[1] for v in FIRST_VIEWS["D2"]]
    P = depth_frame(0, mode, filtered)["P"]
    ref, bad = DS.step_gradient(views, 2, P["positions"]), DS.step_gradient(views, 2, P["positions"], miss=["no_mean_term"])
    hit = [k for k in S.SMALL if moved(ref[k], bad[k])]
    assert hit == ["positions", "rotations"], hit
    plain = S.step_gradient(views, 2, P["positions"])
    assert all(np.array_equal(ref[k], plain[k]) for k in ref)


# ---- 3. the conditions hold for the reference alone ----
@pytest.mark.parametrize("name", list(CONFIGS))
def test_conditions_hold_on_the_prepared_scene(name):
    mode, filtered, lams = CONFIGS[name]
    shares = {}
    for v in range(VIEWS):
        f = depth_frame(v, mode, filtered)
        cond = DS.conditions(mode, f["fr"], f["ref"]["contrib"], f["tg"], f["ref"], f["slopes"])
        DS.assert_conditions(mode, cond, f"{name} view {v}", view=v)
        half, view = halves(f, lams)
        assert half["ties"].mean() <= DS.MAX_SIGN_TIES
        sh = DS.term_share(view)
        print(f"\n{name} view {v}: {cond}, term share of sum|g| " + ", ".join(f"{k} {x:.2f}" for k, x in sh.items()))
        for k in ("dL_dmean3D",) + (() if mode == "median" else ("dL_drot",)):
            shares[k] = min(shares.get(k, np.inf), sh.get(k, 0.0))
    assert min(shares.values()) >= MIN_SHARE, shares
    if filtered:
        f = depth_frame(0, mode, filtered)
        assert DS.flat_raw_round_filtered(f["P"], f["f3d"]) >= MIN_FLAT_TO_ROUND
