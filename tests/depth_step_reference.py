"""
The float64 statement of the three --depth-render terms of examples/train.py -- median, plane, plane-median -- as train_view composes
them with a step's other terms.  Test helper like tests/step_reference.py, not a test file: it imports the stages' yardsticks
(step_reference, median_depth_reference, plane_depth_reference, plane_median_reference, normal_render_reference, f64_reference), edits
none of them and writes no mathematics of its own: what is stated here is which yardstick is fed what, and where its result goes.
Two halves, split where the trainer splits them.

Image half (image_half): the captured float32 depth image of the mode -- the median inverse depth, the plane-depth image, the plane
median -- and the captured contributor image, an exact input as in the kernel tests (a float32 / float64 tie never enters), with the
target, the target's mask and lam_d give the mode's cotangent image

    g = lam_d sign_plus(x - t) mask [contrib > 0] / (W H)                      (median, plane-median; sign(0) = +1 as the L1 kernels have it)
    g = lam_d sign_plus(x - t) mask / (W H)  +  the consistency term's gD       (plane)

The L1 is divided by W H, never by the mask's count.  Under `plane` the consistency term's depth normals are those of the PLANE image
(step_reference.consistency_images evaluated on it), its depth-side gradient joins g and not dL_ddepth_image, and without lam_d the
plane image is rendered for that term alone (g is then the consistency part).  The remaining terms are step_reference.image_half's
with the expected-depth L1 switched off: under these modes the depth term writes no dL_ddepth_image; --lambda-normal still does, from
the expected depth.

Parameter half (term_gradients, view_gradients): the term's gradient, ADDED to step_reference.param_half of the remaining terms.  The
frame's lists, the contributor image, the slopes and the cotangent image are exact inputs.
  median         median_depth_reference.gradient_f64's scatter into the inverse-depth leaf, chained through the true z term of
                 1 / depth exactly as step_reference.param_half chains gD.
  plane-median   plane_median_reference.moments_f64, then plane_depth_reference.slopes_vjp_f64 (position and normal), then
                 normal_render_reference.vjp_f64 (rotation; through step_reference.normals_to_rotations_f64, which holds each normal's
                 side).  Nothing goes to scales, opacities or SH.
  plane          plane_depth_reference.yardstick's gradients: its blend columns through f64_reference's geometry VJP and cov3d step, its
                 moments through the same two VJPs as above (classic mode, no filter: what the configurations run).
Under the 3D filter the normal and the flat / round branch are those of the RAW scales (plane_depth.plane_slopes' contract), the
frame is the filtered scene's.  The branch of every Gaussian is read off the captured slopes -- exactly (0, 0) is the fallback -- which
tests/test_gpu_depth_step.py first holds to plane_depth_reference.slopes_f32 of the parameters' raw scales (check_slopes).

step_gradient is the batch mean (1 / n_batch) sum_v including the term.  MISSTATEMENTS names the ways this composition could be
wrong; each is applied to this float64 side only (tests/test_depth_step_reference.py holds every one of them to be visible under the
bounds tests/test_gpu_depth_step.py applies).
"""
import numpy as np
import torch

import f64_reference as F
import features_reference as FR
import median_depth_reference as M
import plane_depth_reference as PD
import plane_median_reference as PM
import step_reference as S

MODES = ("median", "plane", "plane-median")
TERM_KEYS = ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity")
MAX_SIGN_TIES = 1e-3
MAX_MASKED = FR.MAX_MASKED       # the largest share of a view the plane yardstick's pixel mask may cover

MISSTATEMENTS = {
    "has_median_mask_dropped": "the mask is the target's alone",
    "mean_over_mask": "the term is divided by the mask's count, not W H",
    "median_adds_to_expected": "the expected-depth L1 is kept beside the median term",
    "plane_median_not_in_arena": "the view's gradients are taken before the three calls add",
    "plane_median_rot_dropped": "dL/dnormal is not carried on to the rotations",
    "plane_median_centre_dropped": "column 0 of the moments (the centre's inverse depth) is omitted",
    "filtered_scales_for_the_plane": "the slopes' branch and normal are taken from the filtered scales",
    "consistency_gD_to_expected_under_plane": "under plane, the consistency term's depth-side gradient goes to dL_ddepth_image",
    "no_mean_term": "1 / n_batch is missing on the term's part only",
}
IMAGE_MISS = ("has_median_mask_dropped", "mean_over_mask", "median_adds_to_expected", "consistency_gD_to_expected_under_plane")
PARAM_MISS = ("plane_median_not_in_arena", "plane_median_rot_dropped", "plane_median_centre_dropped", "filtered_scales_for_the_plane")
STEP_MISS = ("no_mean_term",)
# the mode each one is a mis-statement of (tests/test_depth_step_reference.py runs it there)
MODE_OF = {"has_median_mask_dropped": "median", "mean_over_mask": "plane-median", "median_adds_to_expected": "median",
           "plane_median_not_in_arena": "plane-median", "plane_median_rot_dropped": "plane-median", "plane_median_centre_dropped": "plane-median",
           "filtered_scales_for_the_plane": "plane-median", "consistency_gD_to_expected_under_plane": "plane", "no_mean_term": "plane-median"}


def _miss(miss):
    miss = set(miss or ())
    unknown = miss - set(MISSTATEMENTS)
    assert not unknown, f"unknown mis-statements {unknown}"
    return miss


_np64 = S._np64


def frame_of(buf, W, H, invd=None):
    """The frame dict the stage references read (frame_walk_reference.frame_of_buffers) over a forward's buffers; invd: the float32
    inverse depths the kernels read (None: 1 / buffers["depths"])."""
    return PD.frame_of_buffers(buf, W, H, invd)


# ------------------------------------------------------------------------------------------------------------------ image half
def sign_ties(x, t):
    """(H, W) bool: 0 < |x - t| < eps32 |x|, the rounding of x.  (Both are float32 inputs, so a float32 subtraction has the exact
    sign and the set is empty on every frame seen; the cap is asserted all the same.)"""
    x, t = _np64(x), _np64(t)
    d = np.abs(x - t)
    return (d > 0) & (d < S.EPS32 * np.abs(x))


def image_half(mode, frame, tg, cfg, miss=None):
    """mode: one of MODES.  frame: step_reference.image_half's, with "depth_img" (H, W), the mode's captured depth image, and
    "contrib" (H, W) int, the captured contributor image (None under plane).  tg, cfg: step_reference.image_half's.
    Returns step_reference.image_half's dict of the REMAINING terms -- the consistency term's parts included under plane -- and
    "g_term" (H, W): the cotangent image of the mode's depth image, "term_l1": its L1 part, "mask": the L1's mask, "ties"."""
    assert mode in MODES, mode
    miss = _miss(miss)
    x = _np64(frame["depth_img"])
    H, W = x.shape
    lam_d = float(cfg.get("lam_d", 0.0))
    assert cfg.get("depth_loss", "l1") == "l1"
    rest = dict(cfg, lam_d=lam_d if (mode == "median" and "median_adds_to_expected" in miss) else 0.0)
    lam_nc = S.active_weights(cfg)[1]
    if mode == "plane":
        rest["lam_nc"] = 0.0                                            # (stated below, on the plane image)
    res = S.image_half(frame, tg, rest)
    g = np.zeros((H, W))
    mask = np.zeros((H, W))
    ties = np.zeros((H, W), bool)
    if lam_d > 0.0:
        t, mask = _np64(tg["depth_target"], (H, W)), _np64(tg["depth_mask"], (H, W))
        if mode != "plane" and "has_median_mask_dropped" not in miss:
            mask = mask * (np.asarray(frame["contrib"]).reshape(H, W) > 0)
        div = float(mask.sum()) if "mean_over_mask" in miss else float(W * H)
        g = lam_d / div * mask * S._plus_sign(x - t)
        ties = sign_ties(x, t) & (mask > 0)
        res["terms"]["depth"] = g                                       # (image_half_bounds' name for the L1's image)
    res.update(term_l1=g, mask=mask, ties=ties)
    if mode == "plane" and lam_nc > 0.0:
        con = S.consistency_images(dict(frame, dinv=frame["depth_img"]), lam_nc, cfg.get("alpha_min", S.NR.ALPHA_MIN))
        res["kappa_n"] = max(res["kappa_n"], con["kappa"])
        res["terms"].update(consistency_gN=con["gN"], consistency_gD=con["gD"], consistency_gA=con["gA"])
        res.update(near=con["near"], counted=con["counted"], E_f32_gN=con["E_f32_gN"], E_f32_gnd=con["E_f32_gnd"], gN=con["gN"])
        res["gA"] = con["gA"] if res["gA"] is None else res["gA"] + con["gA"]
        if "consistency_gD_to_expected_under_plane" in miss:
            res["gD"] = con["gD"] if res["gD"] is None else res["gD"] + con["gD"]
        else:
            g = g + con["gD"]
    res["g_term"] = g
    return res


def image_half_bounds(mode, res, tg, cfg):
    """step_reference.image_half_bounds, per image: "g_term" from the L1's own bound (the float32 rounding of the exact value) and,
    under plane, the consistency term's gD part and the one float32 addition; "gD" from the expected-depth writers alone; "dpix",
    "gA", "gN" as there."""
    t = res["terms"]
    own = ("depth", "consistency_gD") if mode == "plane" else ("depth",)
    part = lambda names: dict(res, terms={k: v for k, v in t.items() if k in names or k in ("exposure_mag", "exposure_mag_E")})
    out = S.image_half_bounds(res, tg, cfg)
    out["g_term"] = S.image_half_bounds(part(own + ("consistency_gN", "consistency_gA")), tg, cfg)["gD"]
    out["gD"] = S.image_half_bounds(part(tuple(k for k in t if k not in own and not (mode == "plane" and k.startswith("consistency")))), tg, cfg)["gD"]
    return out


# -------------------------------------------------------------------------------------------------------------- parameter half
def chosen_ids(fr, contrib):
    """(H, W) int64: the Gaussian each pixel's contributor names, -1 where it names none (plane_median_reference.chosen's rule)."""
    return PM.chosen(fr, np.zeros((fr["N"], 2), np.float32), contrib)["ids"]


def _camera(cam):
    return np.asarray(cam["world_to_camera"], np.float32).reshape(4, 4), float(cam["tan_fovx"]), float(cam["tan_fovy"]), int(cam["width"]), int(cam["height"])


def _moments_to_parameters(P, cam, normals, fallback, mom, rot=True):
    """(dL_dmean3D, dL_drot) of the three plane moments: plane_depth_reference.slopes_vjp_f64, then the normals' VJP."""
    view, tx, ty, W, H = _camera(cam)
    n = int(np.asarray(P["positions"]).reshape(-1, 3).shape[0])
    pos = np.ascontiguousarray(_np64(P["positions"]), np.float32).reshape(n, 3)
    dmean, dn, _, _ = PD.slopes_vjp_f64(normals, None, pos, view, tx, ty, W, H, fallback, mom)
    drot = S.normals_to_rotations_f64(P, cam, normals, dn) if rot else np.zeros((n, 4))
    return dmean, drot, dn


def term_gradients(mode, P, cam, pre, fr, g, contrib=None, slopes=None, normals=None, filter_3d=None, miss=None, nb=None, image=None):
    """The term's own gradient, float64 numpy by TERM_KEYS (zeros where the term does not reach), of sum_p g[p] image[p]:
    g (H, W) the cotangent of the mode's image, contrib the contributor image, slopes (N, 2) the captured float32 slopes, normals
    (N, 3) the float64 normals of the RAW scales (step_reference.gaussian_normals_f64); pre: the float64 preprocess of the scene the
    frame was rendered from; nb: the frame's buffers (plane: what plane_depth_reference.yardstick reads).  Also "masked": the share
    of pixels the plane yardstick left out, "moments".  image (plane): the captured plane image.  The yardstick zeroes the cotangent
    at the pixels of its mask -- a decision of the walk, or a clamp, too near its threshold for float64 to take the kernel's side --
    and the kernel tests zero it there on both sides; a training step cannot, so with `image` those few pixels are stated by the
    float32 restatement of the same header, plane_depth_reference.render_backward_f32, fed the cotangent at them alone."""
    miss = _miss(miss)
    N, H, W = fr["N"], fr["H"], fr["W"]
    out = {"dL_dmean3D": np.zeros((N, 3)), "dL_dscale": np.zeros((N, 3)), "dL_drot": np.zeros((N, 4)), "dL_dopacity": np.zeros(N), "masked": 0.0}
    g = _np64(g, (H, W))
    if mode == "median":
        ids = chosen_ids(fr, contrib)
        signed, _ = M.gradient_f64(fr, {"contrib": (ids >= 0).astype(np.int64), "ids": ids}, g)
        depth = pre["depth"].detach().numpy()
        invd = np.where(depth > 0, 1.0 / np.where(depth > 0, depth, 1.0), 0.0)
        vis = ~np.asarray(pre["culled"], bool)
        view_z = pre["cam"].view[:3, 2].numpy()                        # z = (m, 1) . view[:, 2]: the true z term of 1 / depth
        out["dL_dmean3D"] = np.where(vis, -(invd ** 2) * signed, 0.0)[:, None] * view_z[None, :]
        return out
    sl = np.asarray(slopes, np.float32).reshape(N, 2)
    fallback = ~(sl != 0).any(1)
    if "filtered_scales_for_the_plane" in miss and filter_3d is not None:
        # the branch by the filtered scales (the normal's axis is the same: the filter's map is monotone per axis)
        view, tx, ty, _, _ = _camera(cam)
        sp = np.asarray(S.scene_of(P, filter_3d)["scales"], np.float32)
        pos = np.ascontiguousarray(_np64(P["positions"]), np.float32).reshape(N, 3)
        fallback = fallback | PD.steps(np.asarray(normals, np.float32), sp, pos, view, tx, ty, W, H, np.float32)["fallback"]
        sl = np.where(fallback[:, None], np.float32(0), sl)
    if mode == "plane-median":
        if "plane_median_not_in_arena" in miss:
            return out
        mom = PM.moments_f64(fr, sl, g, contrib)["signed"]
        if "plane_median_centre_dropped" in miss:
            mom = mom * np.array([0.0, 1.0, 1.0])
        out["dL_dmean3D"], out["dL_drot"], _ = _moments_to_parameters(P, cam, normals, fallback, mom, rot="plane_median_rot_dropped" not in miss)
        out["moments"] = mom
        return out
    assert filter_3d is None, "the plane term is stated for the classic mode without the filter"
    r = PD.yardstick(nb, W, H, fr["invd"], sl, g)
    out["masked"] = float(r["mask"].mean())
    blend = {k: r[k]["signed"] for k in PD.OUTPUTS}
    if image is not None and r["mask"].any():
        left = np.where(r["mask"], g, 0.0).astype(np.float32)
        acc, mom32 = PD.render_backward_f32(fr, sl, left, np.asarray(image, np.float32).reshape(H, W))
        blend = {k: blend[k] + PD.layout(acc, mom32, k) for k in PD.OUTPUTS}
    sc, kw = S.scene_of(P), S.render_kw(cam)
    d2 = torch.zeros(N, 3, dtype=S.D)
    d2[:, :2] = torch.as_tensor(blend["dL_dmean2D"])
    dcon = torch.as_tensor(blend["dL_dconic"])                    # (A, B as stored -- the yardstick's half -- unused, C)
    assert F._sw(None)["conic_b_half"]
    visible = ~pre["culled"]
    m3, _, dcov6, _ = F.geometry_vjp_f64(S._fresh(sc), kw, 3, visible, pre["clamped"], d2, dcon, torch.zeros(N, 3, dtype=S.D))
    dsc, drot = F.cov3d_backward_f64(S._fresh(sc), kw, visible, dcov6)
    mom = blend["dL_dplane_moments"]
    dmean, drot2, _ = _moments_to_parameters(P, cam, normals, fallback, mom)
    out.update(dL_dmean3D=m3.detach().numpy() + dmean, dL_dscale=dsc.detach().numpy(), dL_drot=drot.detach().numpy() + drot2,
               dL_dopacity=blend["dL_dopacity"].reshape(N), moments=mom, yardstick=r)
    return out


def view_gradients(rest, term):
    """A view's gradients: step_reference.param_half's of the remaining terms with the term's ADDED; "term" keeps the term's own."""
    out = dict(rest)
    for k in TERM_KEYS:
        out[k] = rest[k] + term[k].reshape(rest[k].shape)
    out["term"] = {k: term[k] for k in TERM_KEYS}
    return out


def term_share(view):
    """{group: sum |g_term| / sum |g|} of a view_gradients result, for the groups the term reaches."""
    return {k: float(np.abs(view["term"][k]).sum() / max(np.abs(view[k]).sum(), 1e-300)) for k in TERM_KEYS if np.abs(view["term"][k]).max() > 0}


def step_gradient(views, n_batch, positions, miss=None, sh="dense"):
    """The batch mean including the term: step_reference.step_gradient of view_gradients' results."""
    miss = _miss(miss)
    out = S.step_gradient(views, n_batch, positions, sh=sh)
    if "no_mean_term" in miss:
        inv = {v: k for k, v in S.GROUP_OF.items()}
        for k in TERM_KEYS:
            out[inv[k]] = out[inv[k]] + (1.0 - 1.0 / n_batch) * sum(v["term"][k].reshape(out[inv[k]].shape) for v in views)
    return out


# ------------------------------------------------------------------------------------------------------------------ conditions
def conditions(mode, fr, contrib, tg, ref=None, slopes=None):
    """What a view must hold for the checks to mean something, as shares of its pixels (and counts): ref = median_f64(fr)."""
    ref = M.median_f64(fr) if ref is None else ref
    c = np.asarray(contrib).reshape(fr["H"], fr["W"])
    mk = _np64(tg["depth_mask"], c.shape)
    out = {"tie": float(ref["tie"].mean()), "has": float((c > 0).mean()), "crossing": float(((ref["contrib"] > 0) & (ref["T_final"] <= 0.5)).mean()),
           "mask_decides": float(((c == 0) | (mk == 0)).mean()), "contrib_decides": float(((c == 0) & (mk > 0)).mean()),
           "target_decides": float(((c > 0) & (mk == 0)).mean())}
    if mode == "plane-median":
        ch = PM.chosen(fr, slopes, c)
        sel = ch["ids"] >= 0
        out["clamped"] = int((sel & ch["clamped"]).sum())
        out["free"] = int((sel & ~ch["clamped"] & (np.asarray(slopes)[np.where(sel, ch["ids"], 0)] != 0).any(2)).sum())
    return out


# A flat disc's footprint is foreshortened along its own slope, so a chosen entry meets the clamp only where the forward's footprint is
# not the disc's own -- f64_reference's Q1, the view rotation taken transposed.  The first orbit view's rotation is symmetric: no
# preparation tried gave it a clamped entry (0 of 1 900 chosen, where the other views had 30 to 150), so it is the one view excused.
NO_CLAMP_VIEW = 0


def assert_conditions(mode, cond, who="", view=None):
    assert cond["tie"] <= M.MAX_TIES, (who, cond)
    if mode != "plane":
        assert cond["has"] >= 0.30 and cond["crossing"] >= 0.05 and cond["mask_decides"] >= 0.05, (who, cond)
        assert cond["contrib_decides"] > 0 and cond["target_decides"] > 0, (who, cond)      # each factor of the mask decides something
    if mode == "plane-median":
        assert cond["free"] >= PM.MIN_FREE, (who, cond)
        if view != NO_CLAMP_VIEW:
            assert cond["clamped"] >= PM.MIN_CLAMPED, (who, cond)


def flat_raw_round_filtered(P, filter_3d):
    """How many Gaussians are flat by their raw scales and round by their filtered ones (plane_depth_reference's step 5, float32)."""
    flat = lambda s: np.sort(np.asarray(s, np.float32), 1)[:, 0] <= PD.MAX_FLATNESS * np.sort(np.asarray(s, np.float32), 1)[:, 1]
    n = int(np.asarray(P["positions"]).reshape(-1, 3).shape[0])
    raw = np.asarray(P["scales"], np.float32).reshape(n, 3)
    return int((flat(raw) & ~flat(np.asarray(S.scene_of(P, filter_3d)["scales"], np.float32))).sum())
