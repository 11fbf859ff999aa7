"""
The float64 statement of one training step of examples/train.py, all terms together.  Test helper like tests/f64_reference.py, not
a test file: it imports the per-stage yardsticks (and edits none of them) and states how the trainer composes them, in two halves
split at the images the trainer hands to backward_view: three cotangent images and, for the two regularisers whose gradient no
image carries, dL_ddistortion and dL_dnormal_image.

Image half (image_half): one view's rendered image, inverse depth and final_T -- the float32 arrays the trainer rendered, widened --
with that view's targets, weights, exposure matrix and the run's lambdas give (dpix, gD, gA, g_dist, gN) of

    L_v = (1 - lam) L1_w(E I) + lam (1 - SSIM_w(E I)) + lam_d depth(Dinv) + lam_a L1(1 - T, A*) + lam_n normal(Dinv, T)
          + lam_dist mean_p Dist(p) + lam_nc consistency(N, Dinv, T)

where Dist is the depth-distortion image (include/gsr_distortion.h; its cotangent is the constant float32(lam_dist / (W H)), held
exactly), consistency is (1 / W H) sum over the counted pixels of 1 - n_d . N / |N| (include/gsr_normal_render.h (e)) with N the
captured normal image -- a fourth exact input -- whose gradient goes to both sides: gN to the normal image, and through the depth
normals' VJP a further pair of gD / gA images ADDED to the other terms'; each of the two acts from its start iteration on
(cfg "dist_from_iter", "nc_from_iter", "it"); depth is the masked L1 (/ W H) or 1 - the Pearson correlation, the alpha and normal terms are normalised by W H, and the
colour term by 3 W H or, under per-pixel weights m, by 3 M.  The exposure backward applies to the colour gradient only; sign(0) = +1
as the L1 kernels have it.  objective() is the same L_v as one differentiable torch scalar, for the autograd check.

Parameter half (param_half): the parameters, the view's camera, the modes, the frame's own lists and the three cotangent images as
exact inputs give the view's gradients in the reference's convention: f64_reference's blend differentiated tile by tile with the
inverse depth a leaf and the alpha image 1 - T included, its geometry VJP and cov3d step, the true z term of 1 / depth; under the
antialiased mode antialias_reference's rho (the effective opacity, the rho VJP, dL_dopacity times rho); under the 3D filter the
filtered scene substituted and filter3d_reference.transpose_closed applied to dL_dscale / dL_dopacity.  The two regularisers join
the blend's ONE scalar (blend_scalar_grads): g_dist Dist with Dist = A M2 - M1^2 of the blend's own weights and the inverse-depth
leaf, and gN . N with N the blend of the Gaussians' normals, a leaf whose gradient goes on to dL_drot alone through
normal_render_reference.vjp_f64 (nothing to positions or scales; the axis is that of the raw scales under the filter; the few
normals normals_f64 marks undecided take the side the captured float32 normals show).  step_gradient() is the
batch mean (1 / n_batch) sum_v over all five groups, the SH group also from the views' colour-gradient payloads.

camera_gradient_f64 is camera_grad_reference's camera gradient by this module's own two stages in both modes: the blend stage
differentiates the same extended scalar, the geometry stage is camera_grad_reference.geometry's VJP, and in the antialiased mode
rho joins it the way antialias_reference.camera_gradient_aa_f64 has it for dpix.  The Gaussians' normals are constants of the
camera there -- the library's stated contract -- and camera_gradient_full_f64 adds their direct dependence on viewmatrix, only to
measure what the contract leaves out.  pose_gradient_f64 chains the camera gradient to the pose correction xi by central
differences of pose.apply_pose_delta on float64 matrices.

MISSTATEMENTS names the ways this composition could be wrong; each is applied to this float64 side only
(tests/test_step_reference.py holds every one of them to be visible under the bounds tests/test_gpu_train_step.py applies).
"""
import numpy as np
import torch

import adam_reference as A
import antialias_reference as AR
import camera_grad_reference as CR
import depth_corr_reference as DC
import dssim_reference as DS
import exposure_reference as XR
import f64_reference as F
import filter3d_reference as FR
import normal_render_reference as NRR
import normals_reference as NR
import weighted_loss_reference as WR

D = torch.float64
GROUP_OF = {"positions": "dL_dmean3D", "scales": "dL_dscale", "rotations": "dL_drot", "opacities": "dL_dopacity", "shs": "dL_dshs"}
SMALL = ("positions", "scales", "rotations", "opacities")

# Each entry: one way the composition could be wrong (the text says what the mis-stated step does).  Names go to image_half,
# param_half and step_gradient as `miss`, a collection of them; every function ignores the names that are not its own.
MISSTATEMENTS = {
    "normal_gA_dropped": "the normal term's alpha-image gradient is not added to dL_dalpha_image",
    "normal_gD_overwrites": "the normal term's depth-image gradient replaces the depth term's instead of adding to it",
    "exposure_backward_omitted": "dL/d(corrected image) is handed to backward as if it were dL/d(render)",
    "exposure_backward_on_gD": "the exposure backward also scales gD (by the mean column sum of A, depth read as a grey colour)",
    "lambda_on_l1": "the L1 part of the colour loss is weighted lam instead of 1 - lam",
    "no_mean_small": "1 / n_batch is missing on positions, scales, rotations and opacities",
    "no_mean_sh": "1 / n_batch is missing on the SH group only",
    "filter_transposes_omitted": "dL_dscale / dL_dopacity of the filtered scene are returned as those of the raw parameters",
    "raw_scene_under_filter": "the backward is taken of the raw scene although the frame was rendered from the filtered one",
    "rho_omitted_from_dopacity": "dL_dopacity is dL/d(opacity rho), not multiplied by the opacity compensation rho",
    "weights_ignored": "the colour loss ignores the per-pixel weights (the plain 3 W H loss)",
    "dist_term_dropped": "the distortion term's stage does not run: no dL_ddistortion reaches the backward",
    "dist_dm_dropped": "the distortion stage's column 11, dL/dm of the inverse depths, is omitted",
    "dist_mean_missing": "dL/dDist is lam_dist, not lam_dist / (W H)",
    "dist_on_moments_of_depth": "Dist is formed from the view depths, not the inverse depths",
    "consistency_gD_overwrites": "the consistency term's depth-image gradient replaces the other terms' instead of adding to them",
    "consistency_gA_dropped": "the consistency term's alpha-image gradient is not added to dL_dalpha_image",
    "consistency_normal_side_dropped": "the consistency term's gradient on the normal image is not carried: no gN stage",
    "consistency_rot_dropped": "dL/d(gaussian normals) is not carried on to the rotations",
    "from_iter_ignored": "a term with a start iteration acts before it",
    "normals_move_with_the_camera": "the camera gradient also carries the normals' direct dependence on viewmatrix, which the "
                                    "library's contract leaves out (include/gsr_normal_render.h (b))",
}
IMAGE_MISS = ("normal_gA_dropped", "normal_gD_overwrites", "exposure_backward_omitted", "exposure_backward_on_gD", "lambda_on_l1", "weights_ignored")
PARAM_MISS = ("filter_transposes_omitted", "raw_scene_under_filter", "rho_omitted_from_dopacity")
STEP_MISS = ("no_mean_small", "no_mean_sh")
# the two regularisers': those the image half shows (a cotangent image present, absent or moved), and those only the gradients show
TERM_IMAGE_MISS = ("dist_term_dropped", "dist_mean_missing", "consistency_gD_overwrites", "consistency_gA_dropped",
                   "consistency_normal_side_dropped", "from_iter_ignored")
TERM_PARAM_MISS = ("dist_dm_dropped", "dist_on_moments_of_depth", "consistency_rot_dropped")
CAMERA_MISS = ("normals_move_with_the_camera",)


def _miss(miss):
    miss = set(miss or ())
    unknown = miss - set(MISSTATEMENTS)
    assert not unknown, f"unknown mis-statements {unknown}"
    return miss


def _np64(a, shape=None):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    a = a.astype(np.float64)
    return a.reshape(shape) if shape is not None else a


def _plus_sign(d):
    return np.where(d < 0.0, -1.0, 1.0)


# ------------------------------------------------------------------------------------------------------------------ image half
def corrected(img, E):
    """E I in float64: the image the colour loss sees (E None: the render itself)."""
    img = _np64(img)
    return img if E is None else XR.apply_f64(img, E)[0]


def tie_pixels(img, E, target, eps=XR.EPS32):
    """(H, W) bool: pixels with a channel where 0 < |E I - target| < 4 eps32 max(|E I|, |target|).  There the float32 evaluation of
    E I may land on the other side of the target, and sign() with it; such pixels are left out of the dpix comparison."""
    x, y = corrected(img, E), _np64(target).reshape(np.shape(img))
    d = np.abs(x - y)
    return ((d > 0) & (d < 4.0 * eps * np.maximum(np.abs(x), np.abs(y)))).any(-1)


def image_half(frame, tg, cfg, miss=None):
    """frame: {"img" (H, W, 3), "dinv" (H, W), "final_T" (H, W), "cam" (tan_fovx, tan_fovy, width, height), "nimg" (H, W, 3): the
            captured normal image, read under lam_nc alone}
    tg:    {"target" (H, W, 3), "weights" (H, W) or None, "E" (12,) or None, "depth_target", "depth_mask", "alpha_target",
            "normal_target" (H, W, 3), "normal_rot" (3, 3) or None} -- only what the lambdas switch on is read
    cfg:   {"lam", "window", "lam_d", "depth_loss" ("l1" / "pearson"), "lam_a", "lam_n", "alpha_min", "lam_dist", "lam_nc",
            "dist_from_iter", "nc_from_iter", "it"}
    Returns {"dpix", "gD", "gA" (float64; gD / gA None when no term writes them), "g_dist" (H, W), "gN" (H, W, 3) (None when the
    term is off or not yet started; with gN also "near", "counted", "E_f32_gN", "E_f32_gnd" of consistency_images), "dE" (12,) or
    None, "g_col" (the gradient with
    respect to the corrected image), "terms": {name: the float64 gradient image of one term, before any sum}, "kappa_n"}."""
    miss = _miss(miss)
    img, dinv, fT = _np64(frame["img"]), _np64(frame["dinv"]), _np64(frame["final_T"])
    H, W = dinv.shape
    img = img.reshape(H, W, 3)
    lam, window = float(cfg.get("lam", 0.0)), cfg.get("window", "gaussian")
    E = tg.get("E")
    x, y = torch.as_tensor(corrected(img, E)), torch.as_tensor(_np64(tg["target"], (H, W, 3)))
    w = tg.get("weights")
    if w is not None and "weights_ignored" not in miss:
        m = torch.as_tensor(_np64(w, (H, W)))
        g_l1 = WR.pixel_grad(x, y, m, 0.0, window)
        g_ss = WR.pixel_grad(x, y, m, 1.0, window) if lam > 0.0 else torch.zeros_like(g_l1)
    else:
        g_l1 = DS.pixel_grad(x, y, 0.0, window)
        g_ss = DS.pixel_grad(x, y, 1.0, window) if lam > 0.0 else torch.zeros_like(g_l1)
    c_l1 = lam if "lambda_on_l1" in miss else 1.0 - lam
    terms = {"colour_l1": c_l1 * g_l1.numpy(), "colour_ssim": lam * g_ss.numpy()}
    g_col = terms["colour_l1"] + terms["colour_ssim"]
    dpix, dE = g_col, None
    if E is not None:
        d_img, dE, mag_img, mag_E = XR.backward_closed(img, E, g_col)
        terms["exposure_mag"], terms["exposure_mag_E"] = mag_img, mag_E
        if "exposure_backward_omitted" not in miss:
            dpix = d_img
    gD = gA = None
    lam_d, lam_a, lam_n = float(cfg.get("lam_d", 0.0)), float(cfg.get("lam_a", 0.0)), float(cfg.get("lam_n", 0.0))
    if lam_d > 0.0:
        t, mk = _np64(tg["depth_target"], (H, W)), _np64(tg["depth_mask"], (H, W))
        if cfg.get("depth_loss", "l1") == "pearson":
            terms["depth"] = DC.closed_form(dinv, t, mk, lam_d)[1]
        else:
            terms["depth"] = lam_d / (W * H) * mk * _plus_sign(dinv - t)
        gD = terms["depth"]
    if lam_a > 0.0:
        alpha32 = (np.float32(1.0) - np.asarray(_np64(frame["final_T"]), np.float32)).astype(np.float64)   # 1 - T as the kernel forms it
        terms["alpha"] = lam_a / (W * H) * _plus_sign(alpha32 - _np64(tg["alpha_target"], (H, W)))
        gA = terms["alpha"]
    kappa_n = 0.0
    if lam_n > 0.0:
        cam = {k: frame["cam"][k] for k in ("tan_fovx", "tan_fovy", "width", "height")}
        cam = NR.camera(cam["width"], cam["height"], cam["tan_fovx"], cam["tan_fovy"])
        d32, t32 = np.asarray(dinv, np.float32), np.asarray(fT, np.float32)
        case = {"Dinv": d32, "final_T": t32, "cam": cam, "dec": NR.decide(d32, t32, cam, cfg.get("alpha_min", NR.ALPHA_MIN)),
                "target": np.asarray(_np64(tg["normal_target"], (H, W, 3)), np.float32), "R": tg.get("normal_rot"), "mask": None,
                "weight32": float(np.float32(lam_n / (W * H)))}
        ref = NR.reference(case)
        kappa_n = NR.kappa(case)
        terms["normal_gD"], terms["normal_gA"] = ref["gD"], ref["gA"]
        gD = ref["gD"] if (gD is None or "normal_gD_overwrites" in miss) else gD + ref["gD"]
        if "normal_gA_dropped" not in miss:
            gA = ref["gA"] if gA is None else gA + ref["gA"]
        elif gA is None:
            gA = np.zeros((H, W))
    lam_dist, lam_nc = active_weights(cfg, miss)
    g_dist = gN = None
    extra = {}
    if lam_dist > 0.0 and "dist_term_dropped" not in miss:            # one torch.full on the GPU side: held exactly
        g_dist = np.full((H, W), float(np.float32(lam_dist if "dist_mean_missing" in miss else lam_dist / (W * H))))
        terms["dist_g"] = g_dist
    if lam_nc > 0.0:
        con = consistency_images(frame, lam_nc, cfg.get("alpha_min", NR.ALPHA_MIN))
        kappa_n = max(kappa_n, con["kappa"])
        terms["consistency_gN"], terms["consistency_gD"], terms["consistency_gA"] = con["gN"], con["gD"], con["gA"]
        extra = {"near": con["near"], "counted": con["counted"], "E_f32_gN": con["E_f32_gN"], "E_f32_gnd": con["E_f32_gnd"]}
        if "consistency_normal_side_dropped" not in miss:
            gN = con["gN"]
        gD = con["gD"] if (gD is None or "consistency_gD_overwrites" in miss) else gD + con["gD"]
        if "consistency_gA_dropped" not in miss:
            gA = con["gA"] if gA is None else gA + con["gA"]
        elif gA is None:
            gA = np.zeros((H, W))
    if "exposure_backward_on_gD" in miss and E is not None and gD is not None:
        gD = gD * (XR.split(E)[0].sum() / 3.0)
    return {"dpix": dpix, "gD": gD, "gA": gA, "g_dist": g_dist, "gN": gN, "dE": dE, "g_col": g_col, "terms": terms, "kappa_n": kappa_n, **extra}


def active_weights(cfg, miss=()):
    """(lam_dist, lam_nc) at iteration cfg["it"]: a term acts from its start iteration on (cfg["dist_from_iter"], cfg["nc_from_iter"])."""
    it = int(cfg.get("it", 0))
    on = lambda lam, start: float(cfg.get(lam, 0.0)) if (it >= int(cfg.get(start, 0)) or "from_iter_ignored" in miss) else 0.0
    return on("lam_dist", "dist_from_iter"), on("lam_nc", "nc_from_iter")


def consistency_images(frame, lam_nc, alpha_min):
    """The depth-normal consistency term of one frame (include/gsr_normal_render.h (e)) from its captured normal image frame["nimg"]
    (float32, widened: an exact input like the other three images): gN by normal_render_reference.consistency_f64 against the float64
    depth normals (validity is normals_reference.decide's float32 decision), and its gnd through the depth normals' float64 VJP to
    (gD, gA).  E_f32_gN / E_f32_gnd: the error of consistency_f32 on this frame -- fed the float32 depth normals of
    normals_reference's float32 gather, as the kernel is fed the normals kernel's -- in units of max|.| over the pixels that are
    not `near` the length threshold: the E_f32 of test_gpu_normal_render (e).  kappa: normals_reference.kappa of the frame."""
    dinv, fT = _np64(frame["dinv"]), _np64(frame["final_T"])
    H, W = dinv.shape
    c = frame["cam"]
    cam = NR.camera(c["width"], c["height"], c["tan_fovx"], c["tan_fovy"])
    d32, t32 = np.asarray(dinv, np.float32), np.asarray(fT, np.float32)
    dec = NR.decide(d32, t32, cam, alpha_min)
    case = {"Dinv": d32, "final_T": t32, "cam": cam, "dec": dec}
    valid = dec["valid"].astype(np.float32)
    nimg = np.asarray(_np64(frame["nimg"], (H, W, 3)), np.float32)
    with torch.no_grad():
        nd = NR.torch_normals(torch.as_tensor(d32.astype(np.float64)), torch.as_tensor(dec["A"].astype(np.float64)), dec, cam).numpy()
    r = NRR.consistency_f64(nimg, nd, valid, None, lam_nc, W, H)
    _, gD, gA = NR.autograd_vjp(case, r["gnd"])
    nd32 = NR.gather(d32, dec, cam, np.zeros((H, W, 3), np.float32), np.float32)[0]
    _, gN32, gnd32, _ = NRR.consistency_f32(nimg, nd32, valid, None, lam_nc, W, H)
    keep = ~r["near"]
    rel = lambda a32, a64: float(np.abs(a32 - a64)[keep].max() / max(np.abs(a64).max(), 1e-300))
    return {"gN": r["gN"], "gD": gD, "gA": gA, "gnd": r["gnd"], "near": r["near"], "counted": r["counted"], "kappa": NR.kappa(case),
            "E_f32_gN": rel(gN32, r["gN"]), "E_f32_gnd": rel(gnd32, r["gnd"])}


def objective(img, dinv, fT, frame, tg, cfg, dist=None, nimg=None):
    """L_v as one float64 torch scalar, differentiable in the tensors img (H, W, 3), dinv and fT (H, W), and, with their terms on,
    the distortion image dist (H, W) and the normal image nimg (H, W, 3).  The normals' validity pattern, the alpha image's sign
    and the consistency term's counted pixels come from the float32 frame, as in image_half."""
    H, W = dinv.shape
    lam, window = float(cfg.get("lam", 0.0)), cfg.get("window", "gaussian")
    E = tg.get("E")
    x = img
    if E is not None:
        Am, b = XR.split(E)
        x = img @ torch.as_tensor(Am) + torch.as_tensor(b)
    y = torch.as_tensor(_np64(tg["target"], (H, W, 3)))
    if tg.get("weights") is not None:
        L = WR.loss(x, y, torch.as_tensor(_np64(tg["weights"], (H, W))), lam, window)
    else:
        L = DS.loss(x, y, lam, window)
    lam_d, lam_a, lam_n = float(cfg.get("lam_d", 0.0)), float(cfg.get("lam_a", 0.0)), float(cfg.get("lam_n", 0.0))
    if lam_d > 0.0:
        t, mk = torch.as_tensor(_np64(tg["depth_target"], (H, W))), torch.as_tensor(_np64(tg["depth_mask"], (H, W)))
        if cfg.get("depth_loss", "l1") == "pearson":
            M = mk.sum()
            dr, dt = dinv - (mk * dinv).sum() / M, t - (mk * t).sum() / M
            L = L + lam_d * (1.0 - (mk * dr * dt).sum() / torch.sqrt((mk * dr * dr).sum() * (mk * dt * dt).sum()))
        else:
            L = L + lam_d * (mk * (dinv - t).abs()).sum() / (W * H)
    if lam_a > 0.0:
        L = L + lam_a * ((1.0 - fT) - torch.as_tensor(_np64(tg["alpha_target"], (H, W)))).abs().sum() / (W * H)
    if lam_n > 0.0:
        c = frame["cam"]
        cam = NR.camera(c["width"], c["height"], c["tan_fovx"], c["tan_fovy"])
        d32, t32 = np.asarray(_np64(frame["dinv"]), np.float32), np.asarray(_np64(frame["final_T"]), np.float32)
        dec = NR.decide(d32, t32, cam, cfg.get("alpha_min", NR.ALPHA_MIN))
        th, t_ok = NR.target_unit(np.asarray(_np64(tg["normal_target"], (H, W, 3)), np.float32), tg.get("normal_rot"))
        ok = torch.as_tensor(dec["valid"] & t_ok)
        n = NR.torch_normals(dinv, 1.0 - fT, dec, cam)
        L = L + float(np.float32(lam_n / (W * H))) * torch.where(ok, 1.0 - (n * torch.as_tensor(th)).sum(-1), torch.zeros_like(dinv)).sum()
    lam_dist, lam_nc = active_weights(cfg)
    if lam_dist > 0.0:
        L = L + float(np.float32(lam_dist / (W * H))) * dist.sum()
    if lam_nc > 0.0:
        c = frame["cam"]
        cam = NR.camera(c["width"], c["height"], c["tan_fovx"], c["tan_fovy"])
        d32, t32 = np.asarray(_np64(frame["dinv"]), np.float32), np.asarray(_np64(frame["final_T"]), np.float32)
        dec = NR.decide(d32, t32, cam, cfg.get("alpha_min", NR.ALPHA_MIN))
        n32 = np.asarray(_np64(frame["nimg"], (H, W, 3)), np.float32)
        L2 = (n32[..., 0] * n32[..., 0] + n32[..., 1] * n32[..., 1]) + n32[..., 2] * n32[..., 2]
        counted = torch.as_tensor(dec["valid"] & (L2 >= NRR.MIN_LENGTH * NRR.MIN_LENGTH))
        nd = NR.torch_normals(dinv, 1.0 - fT, dec, cam)
        ln = torch.where(counted, nimg.norm(dim=2), torch.ones_like(dinv))
        L = L + lam_nc / (W * H) * torch.where(counted, 1.0 - (nd * nimg).sum(-1) / ln, torch.zeros_like(dinv)).sum()
    return L


# -------------------------------------------------------------------------------------------------------------- parameter half
def render_kw(cam, bg=(0.0, 0.0, 0.0)):
    """The camera half of the render / backward keywords, as forward.render_view passes a trainer's camera dict (degree 3)."""
    return {"background": np.asarray(bg, np.float32), "viewmatrix": cam["world_to_camera"], "projmatrix": cam["full_proj_matrix"],
            "tan_fovx": cam["tan_fovx"], "tan_fovy": cam["tan_fovy"], "image_height": cam["height"], "image_width": cam["width"],
            "campos": cam["camera_center"], "degree": 3, "scale_modifier": 1.0}


def scene_of(P, filter_3d=None):
    """The scene dict the float64 modules take (means / scales / rotations / opacities / shs), from a trainer's parameter dict of
    float32 arrays.  With filter_3d: scales and opacities are the filtered ones, float64 tensors (filter3d_reference.apply_f64)."""
    n = int(np.asarray(P["positions"]).reshape(-1, 3).shape[0])
    f32 = lambda a, shape: np.ascontiguousarray(_np64(a), np.float32).reshape(shape)
    sc = {"means": f32(P["positions"], (n, 3)), "scales": f32(P["scales"], (n, 3)), "rotations": f32(P["rotations"], (n, 4)),
          "opacities": f32(P["opacities"], (n,)), "shs": f32(P["shs"], (n * 16, 3))}
    if filter_3d is not None:
        with torch.no_grad():
            sp, op = FR.apply_f64(sc["scales"], sc["opacities"], _np64(filter_3d))
        sc["scales"], sc["opacities"] = sp, op
    return sc


def _fresh(sc):
    """A copy whose tensors are fresh leaves (the float64 modules call requires_grad_ on what they are handed)."""
    return {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in sc.items()}


def preprocess(P, cam, rasterize_mode="classic", filter_3d=None):
    """The float64 forward's per-Gaussian half under the run's modes."""
    sc, kw = scene_of(P, filter_3d), render_kw(cam)
    pre = (AR.preprocess_aa_f64 if rasterize_mode == "antialiased" else F.preprocess_f64)(_fresh(sc), kw, 3, 1.0)
    return pre


def brute_force_lists(pre):
    """(point_list, ranges) of a float64 forward: every tile's Gaussians by its rectangle, sorted by depth (ties by index).  For
    the CPU checks of the modes that have no float32 CPU forward; a GPU frame brings its own lists."""
    cam = pre["cam"]
    gx, gy = (cam.W + F.TILE - 1) // F.TILE, (cam.H + F.TILE - 1) // F.TILE
    depth, rect, vis = pre["depth"].detach().numpy(), pre["rect"], ~pre["culled"]
    pl, ranges = [], []
    for ty in range(gy):
        for tx in range(gx):
            inside = np.nonzero(vis & (rect[:, 0] <= tx) & (tx < rect[:, 2]) & (rect[:, 1] <= ty) & (ty < rect[:, 3]))[0]
            inside = inside[np.argsort(depth[inside], kind="stable")]
            ranges.append((len(pl), len(pl) + len(inside)))
            pl.extend(inside.tolist())
    return np.asarray(pl, np.int32), np.asarray(ranges, np.int32).reshape(-1, 2)


def forward_f64(pre, point_list, ranges, rasterize_mode="classic"):
    """(image, inverse depth, final_T, n_contrib) float64 numpy over the given lists."""
    cam = pre["cam"]
    blend = AR.blend_f64 if rasterize_mode == "antialiased" else F.blend_f64
    with torch.no_grad():
        out = blend(pre["xy"], pre["conic"], pre["opacity"], pre["colour"], pre["depth"], point_list, ranges, cam.bg, cam.W, cam.H)
    return tuple(o.numpy() for o in out)


def gaussian_normals_f64(P, cam, captured=None):
    """(n (N, 3) float64, flipped): normal_render_reference.normals_f64 of the RAW scales (the 3D filter's map is monotone per axis:
    the shortest axis is the same), the stored rotations, the positions and the camera's world_to_camera.  The rows it marks
    undecided -- the side a Gaussian faces is a float32 decision where t is near 0 -- take the side the captured float32 normals
    show; at most 1 % of N may be undecided (asserted).  flipped: the rows whose side was taken from `captured`."""
    n = int(np.asarray(P["positions"]).reshape(-1, 3).shape[0])
    f32 = lambda a, shape: np.ascontiguousarray(_np64(a), np.float32).reshape(shape)
    r = NRR.normals_f64(f32(P["scales"], (n, 3)), f32(P["rotations"], (n, 4)), f32(P["positions"], (n, 3)), f32(cam["world_to_camera"], (4, 4)))
    out, und = r["n"].copy(), r["undecided"]
    assert und.mean() <= 0.01, f"{int(und.sum())} of {n} normals undecided"
    flipped = np.zeros(n, bool)
    if captured is not None and und.any():
        flipped = und & ((out * _np64(captured, (n, 3))).sum(1) < 0)
        out[flipped] = -out[flipped]
    return out, flipped


def normals_to_rotations_f64(P, cam, normals, g):
    """dL_drot (N, 4) float64 of dL/d(normals) = g: normal_render_reference.vjp_f64, with the side of each row that of `normals` (the
    VJP is linear in sigma).  Nothing goes to positions, scales or the camera (include/gsr_normal_render.h (b))."""
    n = int(np.asarray(P["positions"]).reshape(-1, 3).shape[0])
    f32 = lambda a, shape: np.ascontiguousarray(_np64(a), np.float32).reshape(shape)
    dq, _, r = NRR.vjp_f64(f32(P["scales"], (n, 3)), f32(P["rotations"], (n, 4)), f32(P["positions"], (n, 3)), f32(cam["world_to_camera"], (4, 4)), g)
    same = (r["n"] * _np64(normals, (n, 3))).sum(1) >= 0
    return dq * np.where(same, 1.0, -1.0)[:, None]


def blend_scalar_grads(tile, leaves, point_list, ranges, W, H, bg, cap_grad, dpix=None, gD=None, gA=None, g_dist=None, gN=None, normals=None,
                       miss=()):
    """The blend stage of both halves: d/d(xy, conic, opacity, colour, 1/depth [, normals]) of the ONE scalar

        sum_p  dpix . C + gD Dinv + gA (1 - T) + g_dist Dist + gN . N

    tile by tile over the frame's lists, `tile` the mode's tile function.  Dist = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2
    (include/gsr_distortion.h) = A M2 - M1^2 with A, M1, M2 the blend of the "colours" (1, m, m^2) over background 0, m the
    inverse-depth leaf; N = sum_k w_k n[i_k] the blend of the normals (a leaf, background 0): both ride the tile function as
    further colour channels, so they see the weights the image was drawn with.  Returns the list of gradients, in the order of
    `leaves`, the normals' last when gN is given."""
    xy, con, op, col, invd = leaves
    wrt = list(leaves)
    cot = lambda a, shape: None if a is None else torch.as_tensor(_np64(a, shape))
    cP, cD, cA, cG, cN = cot(dpix, (H, W, 3)), cot(gD, (H, W)), cot(gA, (H, W)), cot(g_dist, (H, W)), cot(gN, (H, W, 3))
    nl = None
    if cN is not None:
        nl = torch.as_tensor(_np64(normals, (xy.shape[0], 3))).clone().requires_grad_(True)
        wrt.append(nl)
    acc = [torch.zeros_like(t) for t in wrt]
    pl = torch.as_tensor(np.asarray(point_list, dtype=np.int64))
    ext_bg = torch.cat([bg] + [torch.zeros(3, dtype=D)] * ((cG is not None) + (nl is not None)))
    for s, e, yy, xx in F._tiles(W, H, ranges):
        if e <= s:
            continue
        yt, xt = torch.as_tensor(yy), torch.as_tensor(xx)
        chans = [col]                                                   # (a fresh graph per tile: each is differentiated on its own)
        if cG is not None:
            m = invd.detach() if "dist_dm_dropped" in miss else invd
            if "dist_on_moments_of_depth" in miss:
                m = torch.where(invd > 0, 1.0 / torch.where(invd > 0, invd, torch.ones_like(invd)), torch.zeros_like(invd))
            chans += [torch.ones_like(m)[:, None], m[:, None], (m * m)[:, None]]
        if nl is not None:
            chans.append(nl)
        out, inv_d, T, _ = tile(xy, con, op, torch.cat(chans, 1), invd, pl[s:e], xt.to(D), yt.to(D), ext_bg, cap_grad)
        L = torch.zeros((), dtype=D)
        if cP is not None:
            L = L + (out[:, :3] * cP[yt, xt]).sum()
        if cD is not None:
            L = L + (inv_d * cD[yt, xt]).sum()
        if cA is not None:
            L = L + ((1.0 - T) * cA[yt, xt]).sum()
        k = 3
        if cG is not None:
            L = L + ((out[:, 3] * out[:, 5] - out[:, 4] ** 2) * cG[yt, xt]).sum()
            k = 6
        if nl is not None:
            L = L + (out[:, k:k + 3] * cN[yt, xt]).sum()
        if not L.requires_grad:
            continue
        for a, g in zip(acc, torch.autograd.grad(L, wrt, allow_unused=True)):
            if g is not None:
                a += g
    return acc


def regulariser_images_f64(pre, point_list, ranges, rasterize_mode="classic", normals=None):
    """(Dist (H, W), N (H, W, 3)) float64 numpy of the float64 forward over the given lists: the distortion image as A M2 - M1^2 and
    the blend of `normals` (zeros without), by the mode's tile function with (1, m, m^2, n) as colours over background 0."""
    cam, N = pre["cam"], pre["N"]
    tile = AR._blend_tile if rasterize_mode == "antialiased" else F._blend_tile
    depth = pre["depth"].detach()
    m = torch.where(depth > 0, 1.0 / torch.where(depth > 0, depth, torch.ones_like(depth)), torch.zeros_like(depth))
    nn = torch.zeros(N, 3, dtype=D) if normals is None else torch.as_tensor(_np64(normals, (N, 3)))
    chans = torch.cat([torch.ones(N, 1, dtype=D), m[:, None], (m * m)[:, None], nn], 1)
    dist, nimg = np.zeros((cam.H, cam.W)), np.zeros((cam.H, cam.W, 3))
    pl = torch.as_tensor(np.asarray(point_list, dtype=np.int64))
    with torch.no_grad():
        for s, e, yy, xx in F._tiles(cam.W, cam.H, ranges):
            if e <= s:
                continue
            out = tile(pre["xy"], pre["conic"], pre["opacity"], chans, m, pl[s:e], torch.as_tensor(xx).to(D), torch.as_tensor(yy).to(D),
                       torch.zeros(6, dtype=D), True)[0]
            dist[yy, xx] = (out[:, 0] * out[:, 2] - out[:, 1] ** 2).numpy()
            nimg[yy, xx] = out[:, 3:6].numpy()
    return dist, nimg


def param_half(P, cam, point_list, ranges, dpix, gD=None, gA=None, rasterize_mode="classic", filter_3d=None, miss=None, pre=None,
               g_dist=None, gN=None, normals=None):
    """One view's gradients in the reference's convention, float64 numpy: dL_dmean3D, dL_dscale, dL_drot, dL_dopacity, dL_dshs
    (N * 16, 3), and dL_dcolor (N, 3), the rows of the view's SH payload.  dpix / gD / gA: the cotangent images (None: zero).
    g_dist (H, W): dL/dDist of the distortion term; gN (H, W, 3) with normals (N, 3), the parameters' normals
    (gaussian_normals_f64): dL/d(normal image) of the consistency term -- both join the blend's scalar (blend_scalar_grads), and the
    normals' gradient goes on to dL_drot alone (normals_to_rotations_f64; also returned, as dL_dgaussian_normals)."""
    miss = _miss(miss)
    aa = rasterize_mode == "antialiased"
    filt = filter_3d if "raw_scene_under_filter" not in miss else None
    sc, kw = scene_of(P, filt), render_kw(cam)
    if pre is None or filt is not filter_3d:
        pre = (AR.preprocess_aa_f64 if aa else F.preprocess_f64)(_fresh(sc), kw, 3, 1.0)
    sw = F._sw(None)
    c, N = pre["cam"], pre["N"]
    W, H = c.W, c.H
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    xy, con, op, col = leaf(pre["xy"]), leaf(pre["conic"]), leaf(pre["opacity"]), leaf(pre["colour"])
    depth = pre["depth"].detach()
    invd = leaf(torch.where(depth > 0, 1.0 / torch.where(depth > 0, depth, torch.ones_like(depth)), torch.zeros_like(depth)))
    if "dist_term_dropped" in miss:
        g_dist = None
    if "consistency_normal_side_dropped" in miss:
        gN = None
    acc = blend_scalar_grads(AR._blend_tile if aa else F._blend_tile, (xy, con, op, col, invd), point_list, ranges, W, H, c.bg,
                             sw["alpha_cap_passes_grad"], dpix, gD, gA, g_dist, gN, normals, miss)
    gxy, gcon, gop, gcol, ginvd = acc[:5]
    dL_dmean2D = torch.zeros(N, 3, dtype=D)
    dL_dmean2D[:, 0], dL_dmean2D[:, 1] = gxy[:, 0] * (0.5 * W), gxy[:, 1] * (0.5 * H)
    dL_dconic = torch.zeros(N, 4, dtype=D)
    dL_dconic[:, 0], dL_dconic[:, 3] = gcon[:, 0], gcon[:, 2]
    dL_dconic[:, 1] = gcon[:, 1] * (0.5 if sw["conic_b_half"] else 1.0)
    visible = ~pre["culled"]
    m3, dshs, dcov6, _ = F.geometry_vjp_f64(_fresh(sc), kw, 3, visible, pre["clamped"], dL_dmean2D, dL_dconic, gcol)
    dop = gop
    if aa:
        r_mean, r_cov = AR.rho_vjp_f64(_fresh(sc), kw, visible, pre["opacity_raw"].detach() * gop)
        m3, dcov6 = m3 + r_mean, dcov6 + r_cov
        if "rho_omitted_from_dopacity" not in miss:
            dop = gop * pre["rho"].detach()
    dsc, drot = F.cov3d_backward_f64(_fresh(sc), kw, visible, dcov6)
    vis = torch.as_tensor(np.asarray(visible, dtype=bool))
    view_z = c.view[:3, 2].to(D)                                        # z = (m, 1) . view[:, 2]: the true z term of 1 / depth
    m3 = m3 + torch.where(vis, -(invd.detach() ** 2) * ginvd, torch.zeros_like(ginvd))[:, None] * view_z[None, :]
    dsc, dop = dsc.detach().numpy(), dop.detach().numpy()
    if filter_3d is not None and "filter_transposes_omitted" not in miss:
        raw = scene_of(P)
        dsc, dop, _ = FR.transpose_closed(raw["scales"], raw["opacities"], _np64(filter_3d), dsc, dop)
    n = lambda t: t.detach().numpy()
    drot, dnormals = n(drot), None
    if gN is not None:
        dnormals = n(acc[5])
        if "consistency_rot_dropped" not in miss:
            drot = drot + normals_to_rotations_f64(P, cam, normals, dnormals)
    return {"dL_dmean3D": n(m3), "dL_dscale": dsc, "dL_drot": drot, "dL_dopacity": dop, "dL_dshs": n(dshs), "dL_dcolor": n(gcol),
            "clamped": pre["clamped"], "campos": n(c.campos), "dL_dgaussian_normals": dnormals}


def payload_of(view):
    """A view's SH payload (3 N + 4 floats) from param_half's output: the colour-gradient rows with the clamped channels zero (they
    pass nothing to the coefficients), the camera centre, one unused float."""
    rows = view["dL_dcolor"] * (~np.asarray(view["clamped"], bool))
    return np.concatenate([rows.reshape(-1), view["campos"].reshape(3), [0.0]])


def step_gradient(views, n_batch, positions, miss=None, sh="dense"):
    """The batch-mean gradient by optimizer group from the views' param_half outputs: (1 / n_batch) sum_v, for all five groups.
    sh="dense": the mean of the views' dL_dshs; sh="payloads": adam_reference.sh_gradient_from_views of the views' payloads with
    scale 1 / n_batch (what the factored path hands the Adam kernel as sh_views and sh_scale)."""
    miss = _miss(miss)
    out = {}
    for k in SMALL:
        out[k] = sum(v[GROUP_OF[k]] for v in views) * (1.0 if "no_mean_small" in miss else 1.0 / n_batch)
    s = 1.0 if "no_mean_sh" in miss else 1.0 / n_batch
    if sh == "dense":
        out["shs"] = sum(v["dL_dshs"] for v in views) * s
    else:
        out["shs"] = A.sh_gradient_from_views(positions, [payload_of(v) for v in views], 3, s)
    return out


# ------------------------------------------------------------------------------------------------------------------ the pose
def pose_gradient_f64(P, start_cam, xi, radii, point_list, ranges, dpix, gD=None, gA=None, rasterize_mode="classic", filter_3d=None, h=1e-6,
                      apply_pose_delta=None, g_dist=None, gN=None, normals=None):
    """(dL/dxi (6,), bound scale (6,)) float64 of a frame rendered at apply_pose_delta(start_cam, xi): the camera gradient with
    respect to (viewmatrix, projmatrix, campos), each taken as independent (camera_gradient_f64 below, under the run's modes; the
    filter is held fixed, as the trainer holds it), chained to xi by central differences (step h) of apply_pose_delta on the start
    camera's matrices widened to float64.  The second item chains sum |term| the same way through |d entry / d xi|: what a bound
    on the 35 camera floats relative to their sum |term| becomes on dL/dxi."""
    cam = apply_pose_delta(start_cam, xi)
    sc, kw = scene_of(P, filter_3d), render_kw(cam)
    grad, scale = camera_gradient_f64(_fresh(sc), kw, radii, point_list, ranges, dpix, gD, gA, antialiased=rasterize_mode == "antialiased",
                                      g_dist=g_dist, gN=gN, normals=normals)
    wide = dict(start_cam, world_to_camera=np.asarray(start_cam["world_to_camera"], np.float64),
                proj_matrix=np.asarray(start_cam["proj_matrix"], np.float64))
    out, reach = np.zeros(6), np.zeros(6)
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        hi, lo = apply_pose_delta(wide, np.asarray(xi, np.float64) + d), apply_pose_delta(wide, np.asarray(xi, np.float64) - d)
        diff = lambda key: ((np.asarray(hi[key], np.float64) - np.asarray(lo[key], np.float64)) / (2.0 * h)).reshape(-1)
        jac = np.concatenate([diff("world_to_camera"), diff("full_proj_matrix"), diff("camera_center"), [0.0]])
        out[k], reach[k] = (grad * jac).sum(), (scale * np.abs(jac)).sum()
    return out, reach


# ------------------------------------------------------------------------------------------- the bounds of the image half
# Nothing here is a new constant: each figure is the bound that term's own GPU test holds for its gradient image
# (tests/test_gpu_train_step.py asserts that the two constants copied from test modules still equal theirs).
DSSIM_GRAD_TOL = 6e-5            # tests/test_gpu_dssim.py GRAD_TOL: max|dg| / max|g_f64| of the unweighted colour gradient
WEIGHTED_GRAD_CEILING = 1e-3     # tests/test_gpu_weighted_loss.py GRAD_CEILING
EPS32 = XR.EPS32


def _golden(name):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as f:
        return json.load(f)


def image_half_bounds(res, tg, cfg):
    """{"dpix", "gD", "gA", "g_dist", "gN"}: the absolute error a correct float32 evaluation of image_half's result `res` may show, by the triangle
    inequality over the bounds of the terms' own GPU tests, each scaled by that term's max|.|, plus 2 eps32 sum of max|term| for
    every float32 addition the trainer performs on the images.
      colour     test_gpu_weighted_loss (10 x its recorded margin, at most its ceiling) under weights, else test_gpu_dssim's GRAD_TOL
      exposure   test_gpu_exposure's K eps32 of the closed form's magnitude image, and the colour bound through |A|
      depth L1, alpha L1   test_gpu_aux_grads check 5: the float32 rounding of the exact value
      Pearson    test_gpu_depth_corr's K eps32 max|g|
      normals    test_gpu_normals' K eps32 kappa max|g|, kappa evaluated on this frame
      consistency   "gN": test_gpu_normal_render (e)'s (3 E_f32 + eps32) max|gN|, E_f32 the error of consistency_f32 on this frame
                 (consistency_images); its gD / gA are gnd, held by the same (3 E_f32 + eps32), carried through the depth normals'
                 VJP: (K eps32 + 3 E_f32 + eps32) kappa max|g|, the input's relative error joining the VJP's own K eps32 under the
                 same cancellation factor
    "g_dist" is 0: the distortion cotangent is one constant, held exactly."""
    t = res["terms"]
    mx = lambda a: float(np.abs(a).max()) if a is not None and np.size(a) else 0.0
    tol_col = (min(10.0 * _golden("weighted_loss_margins.json")["kernels"]["grad"], WEIGHTED_GRAD_CEILING)
               if tg.get("weights") is not None else DSSIM_GRAD_TOL)
    b_col = tol_col * mx(res["g_col"])
    out = {"dpix": b_col, "gD": 0.0, "gA": 0.0}
    if tg.get("E") is not None:
        Am = np.abs(XR.split(tg["E"])[0])
        out["dpix"] = _golden("exposure_margins.json")["backward_image"]["K"] * EPS32 * mx(t["exposure_mag"]) + b_col * float(Am.sum(1).max())
    nm = _golden("normals_margins.json")
    parts = {"gD": [], "gA": []}
    if "depth" in t:
        k = _golden("depth_corr_margins.json")["grad"]["K"] if cfg.get("depth_loss", "l1") == "pearson" else 1.0
        parts["gD"].append((k * EPS32 * mx(t["depth"]), mx(t["depth"])))
    if "alpha" in t:
        parts["gA"].append((EPS32 * mx(t["alpha"]), mx(t["alpha"])))
    if "normal_gD" in t:
        parts["gD"].append((nm["gD"]["K"] * EPS32 * res["kappa_n"] * mx(t["normal_gD"]), mx(t["normal_gD"])))
        parts["gA"].append((nm["gA"]["K"] * EPS32 * res["kappa_n"] * mx(t["normal_gA"]), mx(t["normal_gA"])))
    out["g_dist"] = out["gN"] = 0.0
    if "consistency_gN" in t:
        out["gN"] = (3.0 * res["E_f32_gN"] + EPS32) * mx(t["consistency_gN"])
        rel = 3.0 * res["E_f32_gnd"] + EPS32
        parts["gD"].append(((nm["gD"]["K"] * EPS32 + rel) * res["kappa_n"] * mx(t["consistency_gD"]), mx(t["consistency_gD"])))
        parts["gA"].append(((nm["gA"]["K"] * EPS32 + rel) * res["kappa_n"] * mx(t["consistency_gA"]), mx(t["consistency_gA"])))
    for k, ps in parts.items():                                        # (len - 1 float32 additions, each 2 eps32 of the sum of max|term|)
        out[k] = sum(b for b, _ in ps) + (len(ps) - 1) * 2.0 * EPS32 * sum(m for _, m in ps)
    return out


# ------------------------------------------------------------------------------------- the camera gradient under the modes
def camera_gradient_f64(sc, kw, radii, point_list, ranges, dpix=None, gD=None, gA=None, antialiased=False, g_dist=None, gN=None, normals=None,
                        normals_move=False, miss=None):
    """(grad (36,), scale (36,)) in camera_grad_reference.camera_gradient_f64's layout, by this module's own two stages in both
    modes.  The blend stage differentiates blend_scalar_grads' scalar -- the three cotangent images, the distortion term and the
    consistency term's normal image -- with respect to (xy, conic, opacity, colour, 1/depth); the geometry stage is
    camera_grad_reference.geometry's VJP in the camera leaves, per Gaussian.  In the antialiased mode the blend runs on
    opacity * rho and rho joins the geometry stage with cotangent opacity * dL/d(opacity rho), as
    antialias_reference.camera_gradient_aa_f64 has it for dpix alone.

    The Gaussians' normals are CONSTANTS of the camera here.  That is the library's stated contract (include/gsr_normal_render.h (b):
    the normals' direct dependence on viewmatrix is left out of the camera gradient; camera_grad carries the screen-space columns
    alone), not the derivative of the rendered normal image.  normals_move=True adds what the contract leaves out: n = sigma
    (ah @ V[:3, :3]) differentiated in V, with cotangent dL/d(normals) of the blend stage (camera_gradient_full_f64)."""
    normals_move = normals_move or "normals_move_with_the_camera" in _miss(miss)
    cam = CR.Cam(kw)
    sub, idx, N = CR._visible(sc, radii)
    n = int(idx.numel())
    if n == 0:
        return np.zeros(36), np.zeros(36)
    with torch.no_grad():
        geo = CR.geometry(sub, kw, cam, cam.view, cam.proj, cam.campos, 3, 1.0)
        rho = AR._rho_of_camera(sub, kw, cam, cam.view.expand(n, 4, 4), 1.0) if antialiased else None
    xy, con, col, invd = CR._scatter(N, idx, *geo)
    op_raw = F._t(sub["opacities"], (n,))
    op = CR._scatter(N, idx, op_raw * rho if antialiased else op_raw)[0]
    leaves = [x.detach().clone().requires_grad_(True) for x in (xy, con, op, col, invd)]
    grads = blend_scalar_grads(AR._blend_tile if antialiased else F._blend_tile, leaves, point_list, ranges, cam.W, cam.H, cam.bg, True,
                               dpix, gD, gA, g_dist, gN, normals)
    gxy, gcon, gop, gcol, ginv = [g[idx] for g in grads[:5]]
    Vn = cam.view.expand(n, 4, 4).clone().requires_grad_(True)
    Pn = cam.proj.expand(n, 4, 4).clone().requires_grad_(True)
    Cn = cam.campos.expand(n, 3).clone().requires_grad_(True)
    xy, con, col, invd = CR.geometry(sub, kw, cam, Vn, Pn, Cn, 3, 1.0)
    L = (xy * gxy).sum() + (con * gcon).sum() + (col * gcol).sum() + (invd * ginv).sum()
    if antialiased:
        L = L + (AR._rho_of_camera(sub, kw, cam, Vn, 1.0) * (op_raw * gop)).sum()
    if normals_move and gN is not None:
        eye = np.eye(4, dtype=np.float32)
        r = NRR.normals_f64(sub["scales"], sub["rotations"], sub["means"], eye)            # sigma' ah under the identity view
        ah = torch.as_tensor(r["n"])
        n_here = torch.einsum("ni,nij->nj", ah, cam.view.expand(n, 4, 4)[:, :3, :3])
        side = torch.where((n_here * torch.as_tensor(_np64(normals, (N, 3)))[idx]).sum(1) < 0, -1.0, 1.0).to(D)
        L = L + (side[:, None] * torch.einsum("ni,nij->nj", ah, Vn[:, :3, :3]) * grads[5][idx]).sum()
    gV, gP, gC = torch.autograd.grad(L, (Vn, Pn, Cn), allow_unused=True)
    gV, gP, gC = [torch.zeros_like(x) if g is None else g for g, x in zip((gV, gP, gC), (Vn, Pn, Cn))]
    terms = torch.cat([gV.reshape(n, 16), gP.reshape(n, 16), gC, torch.zeros(n, 1, dtype=D)], 1)
    return terms.sum(0).numpy(), terms.abs().sum(0).numpy()


def camera_gradient_full_f64(sc, kw, radii, point_list, ranges, dpix=None, gD=None, gA=None, antialiased=False, g_dist=None, gN=None, normals=None):
    """camera_gradient_f64 with the normals moving with the camera: only to measure what the library's contract leaves out."""
    return camera_gradient_f64(sc, kw, radii, point_list, ranges, dpix, gD, gA, antialiased, g_dist, gN, normals, normals_move=True)
