"""
A whole training step of examples/train.py held to float64, all terms together (tests/step_reference.py), on the MI355X.

The trainer's stage functions are driven in-process, in main()'s order, at the smallest shapes at which every branch is live:
44 x 44 pixels (a 3 x 3 tile grid with partial tiles on both edges), 600 Gaussians (not a multiple of 4, more than one workgroup),
4 views, two iterations.  gsr.render_view and gsr.backward_view are wrapped to record, per call, the view, what the render
returned, the three cotangent images as they arrive at the backward and what the backward returned.

For every view of both iterations of the configurations S1-S5 and S7-S11 (CONFIGS):
  frame        the captured image / inverse depth / final_T meet the float64 forward of the parameters under the run's modes:
               test_f64_reference.check_forward unchanged in the classic mode; under the antialiased mode or the 3D filter (whose
               per-Gaussian opacity the float64 side does not hold bit for bit) its image criteria against the float64 forward of the
               parameters, after radii match exactly (near-integer radii aside, as there).  The float64 side gets the frame's lists.
  image half   the captured (dpix, gD, gA) against step_reference.image_half on the captured images, within
               step_reference.image_half_bounds (the triangle inequality over the terms' own GPU bounds); pixels on a sign tie of
               the L1 term are left out of dpix, at most 0.1 % of a view.
  per view     each view's returned gradients (and its SH payload) against its own float64, parity.assert_grad: a stage's failure.
  batch        run.model.grads against the float64 batch mean, parity.assert_grad: the composition's.
  Adam         at iteration 0 (zero moments before) adam_m / adam_v against adam_reference.adam_step of the float64 batch mean,
               with the gradient's band propagated (linearly into m, 2 |g| d + d^2 into v), and every parameter element with
               |G64| > 1e-6 at the float64 step's value within 1 % of lr(it = 0).  For the factored SH group this is where
               sh_views and sh_scale show.
  S2           the stepped view's exposure row against exposure_reference.adam_f64 of the float64 dE; pose.m / 0.1 after a view's
               first step against the float64 dL/dxi; pose.t = the number of iterations that drew the view.
  statistics   S2, S4, S9: model.stats.vis_count = the number of batch views with radii > 0, per Gaussian, exactly.
S7-S11 run the depth-distortion (--lambda-dist) and depth-normal consistency (--lambda-normal-consistency) terms, whose gradient is a
stage of the backward switched on by five keywords (TERM_KW); the recorder also wraps distortion.render_distortion and
normal_render.render_normals and clones those keywords.  S7: distortion with D-SSIM, two views and poses; S8: consistency with all
four writers of gD / gA, dense SH; S9: both under the antialiased mode, the 3D filter, poses, exposure and screen statistics; S10:
both from iteration 1 on (iteration 0 carries none of the keywords and meets the statement without the terms; after the opacity
reset --normal-alpha-min 0.01 keeps the consistency term alive, and the distortion weight is 1e5 there); S11: both under
--capacity with a forced overflow.  The weights are those tests/test_step_reference.py settles.  In addition, per view:
  frame        the captured normal image against the float64 blend of the float64 normals over the frame's lists
               (parity.assert_image); the captured distortion image against float64 by tests/test_gpu_distortion.py check 1,
               E_kernel <= 3 E_f32 + floor in units of 1 + mu / sigma, E_f32 of distortion_reference.forward_f32 on the frame.
  image half   the five keywords present exactly when the statement has the term at that iteration; dL_ddistortion exactly the
               constant; gN within step_reference.image_half_bounds (pixels within 1e-6 of the length threshold aside); gD / gA
               within the extended bounds.
  per view, batch, Adam, pose   as above: the float64 side now includes the terms (their cotangents go to param_half and
               pose_gradient_f64; the normals are constants of the camera, the library's contract).
Four deliberate breaks of train_view were run against these on the MI355X, each in a scratch copy: the consistency term's gA
dropped (S8 fails at image half gA), its gD assigned instead of added (S8, image half gD), --dist-from-iter ignored (S10, the
keywords at iteration 0), normal_param_grad=False (S8, per-view rotations).
Paths: three streams against the serial loop, capacity mode and its overflow re-run against the sized path (iteration 0 of each:
the same parameters exactly; once plain and once with both regularisers on), and 17 views per step factored against --dense-sh.  S6: a pose takes one step per iteration and
view under --capacity, from the frame that did not overflow.

tests/golden/step_margins.json records the worst measured ratio of every assertion against its bound, written on the first device
run when absent; a configuration with no row on file has its rows appended, a key missing from a configuration on file fails.  It is not the bound: with the file present a ratio above 10 x its recorded value fails even below 1.  Recorded
values below NOISE count as NOISE there: S6's figure (two runs whose pose steps are lr against the sign of the same gradient) is
1e-13 of its bound, the float64 rounding of the host's pose arithmetic, which repeats to no factor at all; and a recorded share of
exactly zero elements outside a band leaves the band's own cap as the check.
"""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import adam_reference as A
import distortion_reference as DR
import exposure_reference as XR
import parity
import step_reference as S
import test_f64_reference as R
from test_step_reference import LAMBDA_DIST, LAMBDA_NC, S10_ALPHA_MIN, S10_LAMBDA_DIST

pytestmark = pytest.mark.gpu
MARGINS = os.path.join(ROOT, "tests", "golden", "step_margins.json")
SPREAD_FLOOR = 8e-4          # tests/test_gpu_aux_grads.py SPREAD_FLOOR: the backward's run-to-run spread, of max|g|
CAMERA_TRIP = 8.9e-4         # tests/test_gpu_camera_grads.py TRIP: |kernel - f64| / sum |f64 term| of the 35 camera floats
ROUND = 2.0 ** -23
NOISE = 1e-6                 # recorded ratios below this are rounding noise of float64 host arithmetic, not measurements (module docstring)
COMMON = ["--size", "44", "--gaussians", "600", "--views", "4", "--init", "random", "--print-interval", "1000", "--iterations", "2"]
BOTH = ["--lambda-dist", str(LAMBDA_DIST), "--lambda-normal-consistency", str(LAMBDA_NC)]
CONFIGS = {
    "S1": [],
    "S2": ["--lambda-dssim", "0.2", "--lambda-depth", "0.5", "--lambda-alpha", "0.1", "--lambda-normal", "0.05", "--optimize-exposure",
           "--exposure-noise", "0.2", "--optimize-poses", "--pose-noise-deg", "1", "--filter-3d", "--rasterize-mode", "antialiased",
           "--densify-stat", "screen", "--absgrad", "--occluders", "1", "--mask-occluders"],
    "S3": ["--dense-sh", "--views-per-step", "2", "--depth-loss", "pearson", "--lambda-depth", "1", "--depth-noise", "1", "--lambda-normal", "0.05",
           "--normal-noise", "0.1"],
    "S4": ["--views-per-step", "4", "--view-streams", "3", "--lambda-dssim", "0.2", "--lambda-alpha", "0.1", "--densify-stat", "screen"],
    "S5": ["--capacity", "--views-per-step", "2", "--lambda-dssim", "0.2"],
    "S5k": ["--capacity", "--capacity-initial", "64", "--views-per-step", "2", "--lambda-dssim", "0.2"],
    # the distortion and consistency terms (weights: tests/test_step_reference.py, where each term's share of the gradient is held)
    "S7": ["--lambda-dist", str(LAMBDA_DIST), "--lambda-dssim", "0.2", "--views-per-step", "2", "--optimize-poses", "--pose-noise-deg", "1"],
    "S8": ["--lambda-normal-consistency", str(LAMBDA_NC), "--lambda-normal", "0.05", "--normal-noise", "0.1", "--lambda-depth", "0.5",
           "--lambda-alpha", "0.1", "--dense-sh"],
    "S9": BOTH + ["--rasterize-mode", "antialiased", "--filter-3d", "--optimize-poses", "--pose-noise-deg", "1", "--optimize-exposure",
                  "--exposure-noise", "0.2", "--densify-stat", "screen", "--absgrad"],
    "S10": ["--lambda-dist", str(S10_LAMBDA_DIST), "--lambda-normal-consistency", str(LAMBDA_NC), "--dist-from-iter", "1",
            "--normal-consistency-from-iter", "1", "--normal-alpha-min", str(S10_ALPHA_MIN)],
    "S11": BOTH + ["--capacity", "--capacity-initial", "64", "--views-per-step", "2"],
}
TERM_KW = ("dL_ddistortion", "distortion_moments", "dL_dnormal_image", "gaussian_normals", "normal_image")
S6 = ["--capacity", "--capacity-initial", "64", "--optimize-poses", "--pose-noise-deg", "1"]


def test_the_copied_bounds_are_their_owners():
    import test_gpu_aux_grads
    import test_gpu_camera_grads
    import test_gpu_dssim
    import test_gpu_weighted_loss
    assert SPREAD_FLOOR == test_gpu_aux_grads.SPREAD_FLOOR and CAMERA_TRIP == pytest.approx(test_gpu_camera_grads.TRIP, rel=1e-12)
    assert S.DSSIM_GRAD_TOL == test_gpu_dssim.GRAD_TOL and S.WEIGHTED_GRAD_CEILING == test_gpu_weighted_loss.GRAD_CEILING
    import test_step_reference
    assert test_step_reference.CAMERA_TRIP == CAMERA_TRIP


# ------------------------------------------------------------------------------------------------------------- the margins file
def config_of(key):
    """The configuration a margin row belongs to: its first component, for the path tests the first two."""
    parts = key.split("/")
    return "/".join(parts[:2]) if parts[0] == "paths" else parts[0]


def settle(worst, path=None, note=None):
    """Print the worst ratios of a test and hold them to the record.  A configuration with no row at all on file has its rows
    appended (the file is created when absent); a configuration that is on file must have every key there, and none may exceed
    10 x its recorded value.  Recorded values are never changed.  path, note: another test module's record and its "_note"."""
    path = MARGINS if path is None else path
    print("\nworst ratios against the bounds: " + json.dumps({k: float(f"{v:.3g}") for k, v in sorted(worst.items())}))
    doc = {"_note": note or
                    "worst: the largest measured ratio of each assertion of tests/test_gpu_train_step.py against its bound (<= 1 passes), "
                    "over the views and iterations of the configuration, measured on an MI355X against tests/step_reference.py.  It is "
                    "a record of what was measured, not the bound; a later run fails above 10 x a value", "worst": {}}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    rec = doc["worst"]
    on_file = {config_of(k) for k in rec}
    new = {k: v for k, v in worst.items() if config_of(k) not in on_file}
    for k, v in worst.items():
        if k in new:
            continue
        assert k in rec, f"{k} has no recorded margin in {path}"
        assert v <= 10.0 * max(rec[k], NOISE) or (rec[k] == 0.0 and v <= 1.0), f"{k}: ratio {v:.3g} against its bound, recorded {rec[k]:.3g}"
    if new:
        rec.update(new)
        doc["worst"] = {k: rec[k] for k in sorted(rec)}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)


def keep(worst, key, ratio):
    worst[key] = max(worst.get(key, 0.0), float(ratio))


# ------------------------------------------------------------------------------------------------------------ driving the trainer
@functools.lru_cache(maxsize=None)
def trainer():
    spec = importlib.util.spec_from_file_location("gsr_example_train", os.path.join(ROOT, "examples", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def to_np(x):
    return None if x is None else (x.detach().cpu().numpy().copy() if torch.is_tensor(x) else np.asarray(x).copy())


class Recorder:
    """Wraps gsr.render_view / gsr.backward_view of the trainer's package; `calls` holds one record per rendered frame."""
    BUF = ("radii", "point_offsets", "points_xy_image", "depths", "colors", "cov3Ds", "conic_opacity", "point_list", "ranges", "final_Ts",
           "n_contrib", "clamped_state")
    OUT = ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity", "dL_dshs", "_view_payload", "dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos")

    def __init__(self, T, run, monkeypatch):
        self.calls, self.run = [], run
        render, backward = T.gsr.render_view, T.gsr.backward_view
        render_distortion, render_normals = T.gsr.distortion.render_distortion, T.gsr.normal_render.render_normals
        of_frame = lambda buffers: next((c for c in reversed(self.calls) if c["frame_buf"] is buffers), None)

        def distortion(buffers, *args, **kw):
            out = render_distortion(buffers, *args, **kw)
            call = of_frame(buffers)
            if call is not None:
                call.update(dist=out[0].clone(), moments=out[1].clone())
            return out

        def normals(gn, buffers, *args, **kw):
            out = render_normals(gn, buffers, *args, **kw)
            call = of_frame(buffers)
            if call is not None:
                call.update(nimg=out.clone())
            return out

        def render_view(params, camera, background, **kw):
            out = render(params, camera, background, **kw)
            if params is not run.model.params:                                      # (another run's call, or the hidden scene's)
                return out
            v = next(i for i, c in enumerate(run.views.cams) if c is camera)
            # clones made here are on the view's stream
            self.calls.append({"v": v, "cam": camera, "capacity": kw.get("capacity"), "img": out[0].clone(), "dep": out[1].clone(),
                               "buf": {k: out[2][k].clone() for k in self.BUF}, "frame_buf": out[2]})
            return out

        def backward_view(params, camera, background, buffers, dL_dpixels, **kw):
            call = next((c for c in reversed(self.calls) if c["frame_buf"] is buffers), None)
            if call is None:
                return backward(params, camera, background, buffers, dL_dpixels, **kw)
            clone = lambda t: None if t is None else t.clone()
            # (clones: the trainer's tensors are workspace the next view's calls write again)
            call.update(dpix=clone(dL_dpixels), gD=clone(kw.get("dL_ddepth_image")), gA=clone(kw.get("dL_dalpha_image")),
                        kw=dict(kw, **{k: clone(kw.get(k)) for k in TERM_KW}))
            g = backward(params, camera, background, buffers, dL_dpixels, **kw)
            call["out"] = {k: g[k].clone() for k in self.OUT if g.get(k) is not None}     # (the arena is summed in place later)
            return g

        adam = T.gsr.optimizer.adam_update

        def adam_update(params, *args, **kw):
            adam(params, *args, **kw)
            if params is run.model.params:
                self.after_adam = {k: params[k].clone() for k in A.GROUPS}                   # (density control follows in the same step)

        monkeypatch.setattr(T.gsr, "render_view", render_view)
        monkeypatch.setattr(T.gsr, "backward_view", backward_view)
        monkeypatch.setattr(T.gsr.optimizer, "adam_update", adam_update)
        monkeypatch.setattr(T.gsr.distortion, "render_distortion", distortion)
        monkeypatch.setattr(T.gsr.normal_render, "render_normals", normals)

    def take(self):
        """The calls since the last take(), as numpy."""
        torch.cuda.synchronize()
        out = []
        for c in self.calls:
            H, W = c["cam"]["height"], c["cam"]["width"]
            d = {"v": c["v"], "cam": c["cam"], "capacity": c["capacity"], "img": to_np(c["img"]).reshape(H, W, 3), "dep": to_np(c["dep"]).reshape(H, W),
                 "buf": {k: to_np(t) for k, t in c["buf"].items()}, "out": {k: to_np(t) for k, t in c["out"].items()}}
            for k, shape in (("dpix", (H, W, 3)), ("gD", (H, W)), ("gA", (H, W))):
                d[k] = None if c[k] is None else to_np(c[k]).reshape(shape)
            d["term_kw"] = sorted(k for k in TERM_KW if c["kw"].get(k) is not None)
            for k, src, shape in (("g_dist", "dL_ddistortion", (H, W)), ("gN", "dL_dnormal_image", (H, W, 3)), ("normals32", "gaussian_normals", (-1, 3)),
                                  ("kw_nimg", "normal_image", (H, W, 3)), ("kw_moments", "distortion_moments", (H, W, 4))):
                d[k] = None if c["kw"].get(src) is None else to_np(c["kw"][src]).reshape(shape)
            for k, shape in (("dist", (H, W)), ("moments", (H, W, 4)), ("nimg", (H, W, 3))):
                d[k] = None if c.get(k) is None else to_np(c[k]).reshape(shape)
            out.append(d)
        self.calls = []
        return out


def start(argv, monkeypatch, prepare=None):
    """main()'s stages up to the loop; `prepare(T, run)` runs on the fresh run record, before the filter is computed."""
    T = trainer()
    args = T.parse_args(COMMON + list(argv))
    cloud = T.check_args(args)
    dev, rank, world = T.open_device(args)
    views = T.load_views(args, dev)
    P, init_info = T.init_params(args, dev, cloud)
    run = T.new_run(args, dev, rank, world, views, P, init_info)
    if prepare is not None:
        prepare(T, run)
    if args.filter_3d:
        T.recompute_filter(run, -1, "start")
    torch.cuda.synchronize(dev)
    return T, run, Recorder(T, run, monkeypatch)


def snapshot(run):
    """What a step reads, before it: parameters, filter, exposure and pose state."""
    s = {"P": {k: to_np(run.model.params[k]) for k in A.GROUPS}, "filter": to_np(run.mode_kw.get("filter_3d")),
         "xi": [x.copy() for x in run.pose.xi], "pose_t": list(run.pose.t), "start_cams": list(run.views.start_cams)}
    if run.expo is not None:
        s.update(E=to_np(run.expo.E), expo_m=to_np(run.expo.m), expo_v=to_np(run.expo.v), expo_steps=list(run.expo.steps))
    return s


def step(T, run, rec, it):
    snap = snapshot(run)
    T.train_step(run, it)
    return snap, rec.take()


def targets_of(run, v, E, it):
    V, a = run.views, run.args
    tg = {"target": to_np(V.targets[v]), "weights": to_np(V.weights[v].weights) if V.weights is not None else None, "E": E}
    if a.lambda_depth > 0.0:
        tg.update(depth_target=to_np(V.depth_targets[v]), depth_mask=to_np(V.depth_masks[v]))
    if a.lambda_alpha > 0.0:
        tg["alpha_target"] = to_np(V.alpha_targets[v])
    if a.lambda_normal > 0.0:
        tg.update(normal_target=to_np(V.normal_targets[v]), normal_rot=V.normal_rots[v])
    cfg = {"lam": a.lambda_dssim, "window": a.ssim_window, "lam_d": a.lambda_depth, "depth_loss": a.depth_loss, "lam_a": a.lambda_alpha,
           "lam_n": a.lambda_normal, "alpha_min": a.normal_alpha_min, "lam_dist": a.lambda_dist, "lam_nc": a.lambda_normal_consistency,
           "dist_from_iter": a.dist_from_iter, "nc_from_iter": a.normal_consistency_from_iter, "it": it}
    return tg, cfg


# ------------------------------------------------------------------------------------------------------------------- the checks
def check_frame(call, pre, mode, filtered, worst):
    buf = call["buf"]
    if mode == "classic" and not filtered:
        rep = R.check_forward({"pre": pre, "buf": buf, "img": call["img"], "dep": call["dep"], "f64": R.blend_on_buffers(pre, buf)})
        for k in ("xy", "depth", "cov3D", "conic", "colour"):
            if k + "_model" in rep:
                keep(worst, "frame/" + k + "_model", rep[k + "_model"])
    else:
        ambiguous = R._near(pre["radius_f"]) | R._near(pre["rect_f"]).any(1) | (np.abs(pre["p_view"][:, 2].detach().numpy() - 0.2) < 1e-5)
        ok = (buf["radii"] == pre["radii"]) | ambiguous
        assert ok.all(), f"radii differ from the float64 forward of the stated modes at {np.where(~ok)[0][:8]}"
        assert int((ambiguous & (buf["radii"] > 0)).sum()) <= max(1, R.NEAR_MAX * pre["N"])
        i64, d64, T64, n64 = S.forward_f64(pre, buf["point_list"], buf["ranges"], mode)
        rep = {"image": parity.assert_image("image", call["img"], i64),
               "inv_depth": parity.assert_image("inv_depth", call["dep"], d64, tight=2e-5, loose=5e-3, flip_cap=2.5e-2),
               "final_T": parity.assert_image("final_T", buf["final_Ts"], T64), "n_contrib": parity.assert_counts("n_contrib", buf["n_contrib"], n64)}
    for k in ("image", "inv_depth", "final_T"):
        keep(worst, "frame/" + k + "_flips", rep[k][2] / max(2, int(parity.IMG_FLIP_FRAC * call["dep"].size)))
        keep(worst, "frame/" + k + "_outside_tight", (1.0 - rep[k][0]) / (1.0 - 0.999))


def check_term_frame(call, snap, pre, mode, worst):
    """The frame's two further images: the captured normal image against the float64 blend of the float64 normals of the
    parameters over the frame's lists (parity.assert_image), and the captured distortion image against the float64 Dist on the
    frame's buffers by tests/test_gpu_distortion.py check 1: E_kernel <= 3 E_f32 + floor in units of 1 + mu / sigma, E_f32 of
    distortion_reference.forward_f32 on this frame.  What the backward was handed is what those calls returned.  Returns the
    float64 normals (None without the consistency term)."""
    H, W = call["dep"].shape
    normals = None
    if call["nimg"] is not None:
        normals, flipped = S.gaussian_normals_f64(snap["P"], call["cam"], captured=call["normals32"])
        assert np.array_equal(call["kw_nimg"], call["nimg"])
        n64 = S.regulariser_images_f64(pre, call["buf"]["point_list"], call["buf"]["ranges"], mode, normals)[1]
        rep = parity.assert_image("normal_image", call["nimg"], n64)
        keep(worst, "frame/normal_image_flips", rep[2] / max(2, int(parity.IMG_FLIP_FRAC * call["dep"].size)))
        keep(worst, "frame/normal_image_outside_tight", (1.0 - rep[0]) / (1.0 - 0.999))
    if call["dist"] is not None:
        assert np.array_equal(call["kw_moments"], call["moments"])
        r = DR.moments_f64(call["buf"], W, H)
        E_k, E_32 = DR.forward_error(call["dist"], r), DR.forward_error(DR.forward_f32(call["buf"], W, H)[0], r)
        bound = 3.0 * E_32 + DR.golden()["floor"]["forward"]
        print(f"    view {call['v']}: Dist error {E_k:.3e} (1 + mu / sigma), float32 restatement {E_32:.3e}, max Dist {r['dist'].max():.3e}")
        keep(worst, "frame/dist", E_k / bound)
        assert E_k <= bound and r["dist"].max() > 0, (E_k, E_32)
    return normals


def check_image_half(run, call, E, worst, alive, it=0):
    """`alive`: every term that is switched on must be non-zero (iteration 0; the opacity reset that ends it leaves frames too faint
    for a depth normal, and the normal term's images are then zero on both sides)."""
    tg, cfg = targets_of(run, call["v"], E, it)
    res = S.image_half({"img": call["img"], "dinv": call["dep"], "final_T": call["buf"]["final_Ts"], "cam": call["cam"], "nimg": call["nimg"]}, tg, cfg)
    # the two regularisers: present exactly from their start iterations on, all five keywords or none of a term's
    want = (["dL_ddistortion", "distortion_moments"] if res["g_dist"] is not None else []) + \
           (["dL_dnormal_image", "gaussian_normals", "normal_image"] if res["gN"] is not None else [])
    assert call["term_kw"] == sorted(want), (it, call["term_kw"], want)
    if res["g_dist"] is not None:                                                    # one torch.full: exactly the constant
        assert np.array_equal(call["g_dist"].astype(np.float64), res["g_dist"]) and res["g_dist"].max() > 0
    if res["gN"] is not None:
        b = S.image_half_bounds(res, tg, cfg)["gN"]
        far = ~res["near"]
        assert res["near"].mean() <= 1e-2 and np.array_equal(call["gN"][far & ~res["counted"]], np.zeros_like(call["gN"][far & ~res["counted"]]))
        e = np.abs(call["gN"].astype(np.float64) - res["gN"])[far].max()
        print(f"    view {call['v']}: gN err {e:.3e} (bound {b:.3e}, max {np.abs(res['gN']).max():.3e}, {int(res['counted'].sum())} pixels count)")
        keep(worst, "image/gN", e / b if b > 0 else float(e > 0))
        assert e <= b and (np.abs(res["gN"]).max() > 0 or not alive), ("gN", e, b)
    bounds = S.image_half_bounds(res, tg, cfg)
    ties = S.tie_pixels(call["img"], E, tg["target"])
    assert ties.mean() <= 1e-3, f"{ties.sum()} pixels on a sign tie"
    e = np.abs(call["dpix"].astype(np.float64) - res["dpix"])[~ties].max()
    print(f"    view {call['v']}: dpix err {e:.3e} (bound {bounds['dpix']:.3e}, {int(ties.sum())} ties)", end="")
    keep(worst, "image/dpix", e / bounds["dpix"])
    assert e <= bounds["dpix"], ("dpix", e, bounds["dpix"])
    for k in ("gD", "gA"):
        assert (call[k] is None) == (res[k] is None), k
        if res[k] is not None:
            e = np.abs(call[k].astype(np.float64) - res[k]).max()
            print(f", {k} err {e:.3e} (bound {bounds[k]:.3e}, max {np.abs(res[k]).max():.3e})", end="")
            assert np.abs(res[k]).max() > 0 or not alive, k
            assert not alive or all(np.abs(t).max() > 0 for n, t in res["terms"].items() if n != "colour_ssim" or cfg["lam"] > 0.0), "a term of the loss is dead at this size"
            keep(worst, "image/" + k, e / bounds[k] if bounds[k] > 0 else float(e > 0))
            assert e <= bounds[k], (k, e, bounds[k])
    print()
    return res, tg


def grad_ratios(worst, key, got, ref):
    """parity.assert_grad, with its two measured ratios kept: max err / (2e-2 max|g|), and the share outside the tight band / its cap."""
    ok, rel = parity.assert_grad(key, np.asarray(got).reshape(np.shape(ref)), ref)
    keep(worst, key + "/max", rel / parity.GRAD_REST)
    keep(worst, key + "/outside_tight", (1.0 - ok) / max(1.0 - 0.999, 4.0 / np.size(ref)))


def check_view_gradients(call, v64, dense, worst):
    for k, name in S.GROUP_OF.items():
        if k == "shs" and not dense:
            continue
        assert np.abs(v64[name]).max() > 0, name
        grad_ratios(worst, "view/" + k, call["out"][name], v64[name])
    if dense:                                                                            # (the payload is the factored path's)
        return
    n = v64["dL_dcolor"].shape[0]
    pay = S.payload_of(v64)
    grad_ratios(worst, "view/payload", call["out"]["_view_payload"][:3 * n], pay[:3 * n])
    assert np.array_equal(call["out"]["_view_payload"][3 * n:3 * n + 3], np.asarray(call["cam"]["camera_center"], np.float32)[:3])


def check_adam(run, after_adam, snap, G64, lrs, worst, sign_step_min=1e-6):
    """After iteration 0: the moments against adam_step of the float64 batch mean from zero moments, and the parameters' move
    (`after_adam`: the parameters as the Adam call left them; the step's density control then resets the opacities, as the
    reference does at iteration 0).  sign_step_min: the |G64| above which the float64 step itself is held to be lr against the sign
    of g within 1 % of lr (a statement about the reference, not the kernel): the step is lr g / (|g| + eps + 1e-9), so the exact
    threshold is 99 (eps + 1e-9) = 1.09e-6, a little above the `live` threshold of the kernel's check."""
    zeros = {k: np.zeros_like(snap["P"][k], np.float64) for k in A.GROUPS}
    G = {k: G64[k].reshape(snap["P"][k].shape) for k in A.GROUPS}
    P64, M64, V64 = A.adam_step(snap["P"], G, zeros, zeros, lrs, iteration=0)
    b2 = A._f(0.999)
    for k in A.GROUPS:
        m, v, p = (to_np(d[k]).astype(np.float64) for d in (run.model.adam_m, run.model.adam_v, after_adam))
        grad_ratios(worst, "adam_m/" + k, m, M64[k])                                     # linear in g: the gradient's own bands
        g = np.abs(G[k])
        gmax = g.max()
        err = np.abs(v - V64[k])
        band = lambda d: (1.0 - b2) * (2.0 * g * d + d * d) + 4.0 * ROUND * np.abs(V64[k]).max()
        tight, loose = band(parity.GRAD_ABS * gmax + parity.GRAD_REL * g), band(parity.GRAD_REST * gmax)
        outside = float((err > tight).mean())
        keep(worst, "adam_v/" + k + "/outside_tight", outside / max(1.0 - 0.999, 4.0 / err.size))
        keep(worst, "adam_v/" + k + "/max", float((err / loose).max()))
        assert outside <= max(1.0 - 0.999, 4.0 / err.size) and (err <= loose).all(), f"adam_v {k}"
        live = g > 1e-6
        if k == "rotations":                                                            # the renormalisation couples a quaternion's components
            live = np.broadcast_to(live.reshape(-1, 4).all(1, keepdims=True), (live.size // 4, 4)).reshape(live.shape)
        assert live.any(), k
        move = np.abs(p - P64[k])[live].max() / A._f(lrs[k])
        keep(worst, "adam_step/" + k, move / 0.01)
        assert move <= 0.01, f"{k}: parameters off the float64 step by {move:.3g} lr"
        free = live & (np.abs(P64[k] - (snap["P"][k] - A._f(lrs[k]) * np.sign(G[k]))) <= 0.01 * A._f(lrs[k]))
        signed = live & (g > sign_step_min)
        assert k in ("scales", "rotations", "opacities") or free[signed].mean() > 0.99, k     # a first Adam step: lr against the sign of g
    reset = np.minimum(to_np(after_adam["opacities"]), np.float32(0.01))
    assert np.array_equal(to_np(run.model.params["opacities"]), reset), "iteration 0 ends with the reference's opacity reset"


def s2_prepare(T, run):
    """Both chains away from the identity: a seeded exposure per view, a seeded pose correction per view."""
    rng = np.random.default_rng(12)
    n = len(run.views.cams)
    E = (XR.IDENTITY[None, :] + rng.normal(0, 0.05, (n, 12))).astype(np.float32)
    run.expo.load_state_dict({"E": E.tolist(), "m": np.zeros((n, 12)).tolist(), "v": np.zeros((n, 12)).tolist(), "steps": [0] * n})
    for v in range(n):
        run.pose.xi[v] = np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, 0.005, 3)])
        run.views.cams[v] = T.gsr.pose.apply_pose_delta(run.views.start_cams[v], run.pose.xi[v])


def check_exposure(run, snap, call, res, tg, it, worst):
    v, a = call["v"], run.args
    lr = float(np.float32(XR.decayed_lr(a.exposure_lr_init, a.exposure_lr_final, it, a.iterations)))
    margins = S._golden("exposure_margins.json")
    E64, m64, v64 = XR.adam_f64(snap["E"][v], res["dE"], snap["expo_m"][v], snap["expo_v"][v], lr, snap["expo_steps"][v] + 1,
                                float(np.float32(XR.BETA1)), float(np.float32(XR.BETA2)), float(np.float32(XR.EPS)))
    # dE = c^T g: the kernel's own bound (+ 1 for the float32 weights, as test_gpu_exposure's composition check) and the colour
    # gradient's bound through sum |c|
    tol_col = min(10.0 * S._golden("weighted_loss_margins.json")["kernels"]["grad"], S.WEIGHTED_GRAD_CEILING) if tg["weights"] is not None else S.DSSIM_GRAD_TOL
    c = np.abs(call["img"].astype(np.float64)).reshape(-1, 3)
    reach = np.concatenate([np.repeat(c.sum(0), 3), np.full(3, float(c.shape[0]))]) * tol_col * np.abs(res["g_col"]).max()
    bound_dE = (margins["backward_E"]["K"] + 1.0) * XR.EPS32 * res["terms"]["exposure_mag_E"] + reach
    m = to_np(run.expo.m[v]).astype(np.float64)
    r_m = float((np.abs(m - m64) / ((1.0 - float(np.float32(XR.BETA1))) * bound_dE + 4.0 * ROUND * np.abs(m64).max())).max())
    keep(worst, "exposure/m", r_m)
    assert r_m <= 1.0, ("exposure m", r_m)
    assert run.expo.steps[v] == snap["expo_steps"][v] + 1
    if snap["expo_steps"][v] == 0:                 # a first step moves E by lr against the sign of dE: the gradient's error does not reach it
        r_E = float((np.abs(to_np(run.expo.E[v]) - E64) / (np.abs(E64) + lr)).max() / XR.EPS32 / margins["adam"]["K"])
        keep(worst, "exposure/E", r_E)
        assert r_E <= 1.0 and np.abs(E64 - snap["E"][v]).max() > 0.5 * lr, ("exposure E", r_E)
    others = [u for u in range(len(run.views.cams)) if u != v]
    assert np.array_equal(to_np(run.expo.E)[others], snap["E"][others])


def check_pose(T, run, snap, call, mode, worst, normals=None):
    v = call["v"]
    if snap["pose_t"][v] != 0:
        return
    dxi, reach = S.pose_gradient_f64(snap["P"], snap["start_cams"][v], snap["xi"][v], call["buf"]["radii"], call["buf"]["point_list"],
                                     call["buf"]["ranges"], call["dpix"], call["gD"], call["gA"], rasterize_mode=mode, filter_3d=snap["filter"],
                                     apply_pose_delta=T.gsr.pose.apply_pose_delta, g_dist=call["g_dist"], gN=call["gN"], normals=normals)
    got = run.pose.m[v] / 0.1
    r = float((np.abs(got - dxi) / (CAMERA_TRIP * reach)).max())
    print(f"    view {v}: dL/dxi {np.array2string(dxi, precision=3)} err/bound {r:.3g}")
    keep(worst, "pose/dxi", r)
    assert np.abs(dxi).max() > 0 and r <= 1.0, ("pose", got, dxi)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_train_step_against_float64(name, monkeypatch):
    T, run, rec = start(CONFIGS[name], monkeypatch, s2_prepare if name in ("S2", "S9") else None)
    a = run.args
    mode, dense, worst = a.rasterize_mode, a.dense_sh, {}
    drawn = [0] * len(run.views.cams)
    seen = np.zeros(run.model.num_points, np.int64)
    for it in range(a.iterations):
        snap, calls = step(T, run, rec, it)
        overflowed = {(r["iteration"], r["view"]) for r in run.capacity_log}
        print(f"\n{name} iteration {it}: views {[c['v'] for c in calls]}" + (f", overflowed {sorted(overflowed)}" if overflowed else ""))
        views64, batch, first = [], [], set()
        for call in calls:
            v = call["v"]
            if (it, v) in overflowed and v not in first:                        # the overflowed frame: nothing of it is trusted, or used
                first.add(v)
                assert call["capacity"] is not None
                continue
            filt = snap["filter"]
            pre = S.preprocess(snap["P"], call["cam"], mode, filt)
            check_frame(call, pre, mode, filt is not None, worst)
            normals = check_term_frame(call, snap, pre, mode, worst)
            E = snap["E"][v] if run.expo is not None else None
            res, tg = check_image_half(run, call, E, worst, alive=it == 0 or name == "S10", it=it)
            v64 = S.param_half(snap["P"], call["cam"], call["buf"]["point_list"], call["buf"]["ranges"], call["dpix"], call["gD"], call["gA"],
                               rasterize_mode=mode, filter_3d=filt, pre=pre, g_dist=call["g_dist"], gN=call["gN"], normals=normals)
            check_view_gradients(call, v64, dense, worst)
            if run.expo is not None:
                check_exposure(run, snap, call, res, tg, it, worst)
            if a.optimize_poses:
                check_pose(T, run, snap, call, mode, worst, normals)
            views64.append(v64)
            batch.append(v)
            drawn[v] += 1
            seen += call["buf"]["radii"] > 0
        assert len(batch) == a.views_per_step == len(set(batch))
        G64 = S.step_gradient(views64, len(batch), snap["P"]["positions"], sh="dense" if dense else "payloads")
        for k in A.GROUPS:
            if k != "shs" or dense:
                grad_ratios(worst, "batch/" + k, to_np(run.model.grads[k]), G64[k])
        if it == 0:
            check_adam(run, rec.after_adam, snap, G64, {k: s.get_lr(0, a.iterations) for k, s in run.sched.items()}, worst)
        if run.screen_stats:
            assert np.array_equal(to_np(run.model.stats.vis_count), seen), "vis_count is not the number of batch views that saw each Gaussian"
        if a.optimize_poses:
            assert list(run.pose.t) == drawn, (run.pose.t, drawn)
    if name == "S5":
        assert run.cap["K"] is not None and not run.capacity_log                # sized iteration 0, capacity-mode iteration 1, no overflow
    if name in ("S5k", "S11"):
        # (K = 64 overflows on the step's first view; the re-run grows K, so the views after it may fit)
        assert (run.capacity_log[0]["iteration"], run.capacity_log[0]["capacity"]) == (0, 64) and all(r["D"] > r["capacity"] for r in run.capacity_log)
    settle({f"{name}/{k}": v for k, v in worst.items()})


# ---------------------------------------------------------------------------------------------------------------- paths agree
def first_step_grads(argv, monkeypatch, prepare=None):
    T, run, rec = start(argv, monkeypatch, prepare)
    T.train_step(run, 0)
    torch.cuda.synchronize()
    return run, {k: to_np(run.model.grads[k]).astype(np.float64) for k in S.SMALL}


def spread(worst, key, got, ref):
    for k in S.SMALL:
        e = float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max())
        keep(worst, f"{key}/{k}", e / SPREAD_FLOOR)
        assert e <= SPREAD_FLOOR, (key, k, e)


def test_three_streams_give_the_serial_loops_gradients(monkeypatch):
    base = ["--views-per-step", "4", "--lambda-dssim", "0.2", "--lambda-alpha", "0.1"]
    _, serial = first_step_grads(base + ["--view-streams", "1"], monkeypatch)
    _, streams = first_step_grads(base + ["--view-streams", "3"], monkeypatch)
    worst = {}
    spread(worst, "paths/streams", streams, serial)
    settle(worst)


def test_capacity_mode_and_its_overflow_rerun_give_the_sized_paths_gradients(monkeypatch):
    worst = {}
    # (the second base: both regularisers on -- their stages bound every walk by the capacity, so this is a designed path)
    for tag, base in (("", ["--views-per-step", "2", "--lambda-dssim", "0.2"]), ("_terms", ["--views-per-step", "2", "--lambda-dssim", "0.2"] + BOTH)):
        _, sized = first_step_grads(base, monkeypatch)
        r_cap, cap = first_step_grads(base + ["--capacity", "--capacity-initial", "1000000"], monkeypatch)
        r_over, over = first_step_grads(base + ["--capacity", "--capacity-initial", "64"], monkeypatch)
        assert not r_cap.capacity_log and r_over.capacity_log and r_over.capacity_log[0]["capacity"] == 64
        for r in r_over.capacity_log:                                       # (the re-run grows K: the step's second view may fit)
            assert r["iteration"] == 0 and r["D"] > r["capacity"]
        assert r_over.cap["K"] == -(-5 * r_over.capacity_log[-1]["D"] // 4) >= r_over.cap["max_D"]     # K grew at the last overflow, to 1.25 x its D
        spread(worst, "paths/capacity" + tag, cap, sized)
        spread(worst, "paths/overflow_rerun" + tag, over, sized)
    settle(worst)


def test_seventeen_views_factored_and_dense_give_the_same_sh_moments(monkeypatch):
    """More views than one Adam call takes (dist.MAX_VIEWS_PER_CALL): the factored path rebuilds the SH gradient in chunks.  Kernel
    against kernel."""
    argv = ["--size", "20", "--gaussians", "130", "--views", "17", "--views-per-step", "17"]
    T = trainer()
    assert 17 > T.gsr.dist.MAX_VIEWS_PER_CALL
    out = {}
    for label, extra in (("factored", []), ("dense", ["--dense-sh"])):
        _, run, rec = start(argv + extra, monkeypatch)
        T.train_step(run, 0)
        torch.cuda.synchronize()
        out[label] = {k: to_np(d["shs"]).astype(np.float64) for k, d in (("m", run.model.adam_m), ("v", run.model.adam_v))}
    worst = {}
    for k, tol in (("m", SPREAD_FLOOR), ("v", 2.0 * SPREAD_FLOOR)):
        ref = out["dense"][k]
        assert np.abs(ref).max() > 0
        e = float(np.abs(out["factored"][k] - ref).max() / np.abs(ref).max())
        keep(worst, f"paths/seventeen_views/{k}", e / tol)
        assert e <= tol, (k, e)
    settle(worst)


# ------------------------------------------------------------------------------------------------------------------------- S6
def test_pose_takes_one_step_per_view_under_capacity_from_the_frame_that_counted(monkeypatch):
    T, cap, _ = start(S6, monkeypatch)
    _, sized, _ = start([x for x in S6 if x not in ("--capacity", "--capacity-initial", "64")], monkeypatch)
    worst = {}
    for it in range(cap.args.iterations):
        before = list(cap.pose.t)
        T.train_step(cap, it)
        T.train_step(sized, it)
        grown = [t1 - t0 for t0, t1 in zip(before, cap.pose.t)]
        print(f"\nS6 iteration {it}: pose.t {cap.pose.t} (sized {sized.pose.t}), capacity retries {len(cap.capacity_log)}")
        assert max(grown) <= 1 and sum(grown) == 1, f"pose.t grew by {grown} in one iteration"
        assert cap.pose.t == sized.pose.t
        for v in range(len(cap.pose.xi)):                                       # a step is lr m^ / (sqrt(v^) + eps): errors of g in units of lr
            e = float(np.abs(cap.pose.xi[v] - sized.pose.xi[v]).max() / cap.args.pose_lr)
            keep(worst, "S6/xi", e / CAMERA_TRIP)
            assert e <= CAMERA_TRIP, (it, v, cap.pose.xi[v], sized.pose.xi[v])
    assert any(r["iteration"] == 0 for r in cap.capacity_log), "the forced overflow did not happen"
    assert max(np.abs(x).max() for x in cap.pose.xi) > 0.5 * cap.args.pose_lr
    settle(worst)
