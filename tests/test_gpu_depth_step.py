"""
The three --depth-render terms of examples/train.py -- median, plane, plane-median -- held to float64 inside a whole training step
(tests/depth_step_reference.py over tests/step_reference.py), on the MI355X.  The kernels are held one by one elsewhere
(tests/test_gpu_median_depth.py, tests/test_gpu_plane_depth.py, tests/test_gpu_plane_median.py); this file holds how train_view
composes them: the mask, the keywords that reach backward_view, where the consistency term's depth-side gradient goes under `plane`,
that the plane-median term (three calls AFTER backward_view) is in the arena the batch mean is taken of, and whose scales it reads
under the 3D filter.

The trainer's stage functions are driven in-process with tests/test_gpu_train_step.py's helpers at that file's shapes: 44 x 44 pixels,
600 Gaussians, 4 views; two iterations where Adam is checked (D1, D2), one elsewhere.  DepthRecorder wraps that file's Recorder and
also median_depth.render_median_depth, plane_depth.render_view_plane_depth, plane_depth.render_view_plane_median_depth and
plane_depth.plane_median_gradients: it clones the mode's depth image, contributor, slopes and normals, the new keywords as they arrive
at backward_view, and, under plane-median, the view's gradients AGAIN after plane_median_gradients has returned.  prepare() makes the
terms live with the numbers tests/test_depth_step_reference.py settles: positions pulled towards the centre, scales flattened
(plane_depth_reference.plane_scales) and grown, opacities raised, a rectangle of every depth mask cleared.

Configurations (CONFIGS; all with --lambda-depth LAMBDA_DEPTH --depth-loss l1 except D4):
  D1 median, --lambda-normal, --lambda-alpha, two views    D5 plane-median, --filter-3d --rasterize-mode antialiased
  D2 plane-median, two views, D-SSIM                        D6 plane-median, --capacity with a forced overflow, two views
  D3 plane, consistency and --lambda-normal                 D7 plane-median, four views on three streams
  D4 plane, consistency alone (a zero dL_dplane_depth)      D8 median, --dense-sh, screen statistics
Per view of every iteration:
  frame        test_gpu_train_step.check_frame (and check_term_frame under the consistency term); the captured slopes against
               plane_depth_reference.slopes_f32 of the parameters' RAW scales (check_slopes); the captured contributor is the
               float64 median outside median_depth_reference's tie mask; the mode's image is bit for bit inv_depth[id] of the named
               entry (median) or plane_median_reference.chosen's m (plane-median), and within 3 E_f32 + eps32 of
               plane_depth_reference.yardstick (plane).
  image half   the cotangent image the trainer made against depth_step_reference.image_half within the L1 kernel's own bound
               (step_reference.image_half_bounds; under plane with the consistency part); dpix, gD, gA, gN as there; the keyword
               set at backward_view is exactly the mode's; median_contributor / the contributor handed to plane_median_gradients
               are the rendered one bit for bit.
  per view     the gradients after the term's last writer -- backward_view, or plane_median_gradients -- against the float64 view
               gradient, check_view_gradients unchanged; under plane-median every key but dL_dmean3D and dL_drot keeps
               backward_view's bits.
  batch, Adam  run.model.grads against the float64 batch mean; D1, D2: check_adam at iteration 0.
  D6, D7       iteration-0 gradients against the serial, sized run of the same parameters (spread, SPREAD_FLOOR); D6 must have
               overflowed and re-run.      D8: vis_count exact.
At iteration 0 the conditions of depth_step_reference.assert_conditions hold on every view (ties, pixels with a median, true
crossings, both factors of the mask deciding, free and clamped chosen entries -- the first orbit view excused from the clamped ones,
depth_step_reference.NO_CLAMP_VIEW --, the term's share of sum |g| >= 10 %, 10 flat-raw / round-filtered Gaussians with slopes in D5), and
the views drawn are those the CPU test settled them for (FIRST_VIEWS); iteration 1 follows the opacity reset and has no crossing to show.
Poses stay out: no configuration passes --optimize-poses -- the plane-median term does not reach the camera gradient (no stage of
the backward carries it).

tests/golden/depth_step_margins.json records the worst ratio of every assertion against its bound per configuration, under
test_gpu_train_step.settle's rules: a record, never the bound; a later run fails above 10 x a recorded value.  Each value is the
largest of three runs that each wrote the file afresh (tools/record_depth_step_margins.py says why one run is not enough).

Under `plane` the float64 yardstick leaves out the few pixels of its mask (4 of 1936 on the view D3 and D4 draw); a step cannot zero
the cotangent there as the kernel test does, and with the consistency term's gradient on them 4 % (D3) and 8 % (D4) of the view's
position gradients left the tight band, so depth_step_reference states those pixels by the float32 restatement of the same header.

Five deliberate breaks of train_view were run against this file on the MI355X, each in a scratch copy; each failed where named:
  the mask without (contrib > 0)                                   D1, image half: g_term off by 6.2e-3 against a bound of 7.4e-10
  plane_median_gradients(..., grads=None), its result discarded    D2, per view: view/positions, 79.1 % inside the band, max error
                                                                   0.98 max|g|
  the consistency term's gD added to dL_ddepth_image under plane   D3, image half: g_term off by 4.3e-2 against a bound of 2.6e-6
  render_view_plane_median_depth given the filtered scales         D5, frame: check_slopes, a branch that is not the raw scales'
                                                                   (before check_slopes existed: per view, view/positions, 98.5 %
                                                                   inside the band, max error 0.38 max|g|)
  the filtered scales given to that call AND to                    D5, frame: check_slopes, the same assertion -- render and gradient
  plane_median_gradients                                           agree with each other then, and only the raw scales tell
"""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
import adam_reference as A
import depth_step_reference as DS
import median_depth_reference as M
import plane_depth_reference as PD
import plane_median_reference as PM
import step_reference as S
from test_depth_step_reference import FIRST_VIEWS, LAMBDA_DEPTH, MASK_HOLE, MIN_FLAT_TO_ROUND, MIN_SHARE, prepared_params
from test_gpu_train_step import (check_adam, check_frame, check_term_frame, check_view_gradients, first_step_grads, grad_ratios, keep,
                                 settle, snapshot, spread, start, targets_of, to_np)
from test_step_reference import LAMBDA_NC

pytestmark = pytest.mark.gpu
MARGINS = os.path.join(ROOT, "tests", "golden", "depth_step_margins.json")
NOTE = ("worst: the largest measured ratio of each assertion of tests/test_gpu_depth_step.py against its bound (<= 1 passes), over the views and "
        "iterations of the configuration, measured on an MI355X against tests/depth_step_reference.py.  It is a record of what was measured, "
        "not the bound; a later run fails above 10 x a value")
DEPTH = ["--lambda-depth", str(LAMBDA_DEPTH), "--depth-loss", "l1"]
ONE = ["--iterations", "1"]
CONFIGS = {
    "D1": DEPTH + ["--depth-render", "median", "--lambda-normal", "0.05", "--lambda-alpha", "0.1", "--views-per-step", "2"],
    "D2": DEPTH + ["--depth-render", "plane-median", "--views-per-step", "2", "--lambda-dssim", "0.2"],
    "D3": DEPTH + ONE + ["--depth-render", "plane", "--lambda-normal-consistency", str(LAMBDA_NC), "--lambda-normal", "0.05"],
    "D4": ONE + ["--depth-render", "plane", "--lambda-normal-consistency", str(LAMBDA_NC)],
    "D5": DEPTH + ONE + ["--depth-render", "plane-median", "--filter-3d", "--rasterize-mode", "antialiased"],
    "D6": DEPTH + ONE + ["--depth-render", "plane-median", "--capacity", "--capacity-initial", "64", "--views-per-step", "2"],
    "D7": DEPTH + ONE + ["--depth-render", "plane-median", "--views-per-step", "4", "--view-streams", "3"],
    "D8": DEPTH + ONE + ["--depth-render", "median", "--dense-sh", "--densify-stat", "screen"],
}
# the serial, sized run a path configuration is compared with
SERIAL = {"D6": DEPTH + ONE + ["--depth-render", "plane-median", "--views-per-step", "2"],
          "D7": DEPTH + ONE + ["--depth-render", "plane-median", "--views-per-step", "4", "--view-streams", "1"]}
NEW_KW = ("dL_dmedian_depth", "median_contributor", "dL_dplane_depth", "plane_slopes", "plane_depth_image")
KW_OF = {"median": ["dL_dmedian_depth", "median_contributor"], "plane": ["dL_dplane_depth", "plane_depth_image", "plane_slopes"], "plane-median": []}


def prepare(T, run):
    """The terms made live (tests/test_depth_step_reference.py settles the numbers on the reference alone)."""
    P = run.model.params
    new = prepared_params({k: to_np(P[k]) for k in ("positions", "scales", "opacities")})
    for k, a in new.items():
        P[k].copy_(torch.as_tensor(a).reshape(P[k].shape).to(P[k].device))
    if run.views.depth_masks is not None:
        for m in run.views.depth_masks:
            m[MASK_HOLE] = 0


class DepthRecorder:
    """Over test_gpu_train_step.Recorder (whose wrappers of render_view / backward_view these call): per rendered frame also the
    inverse depths the stages read, what the mode's render returned, the new keywords at backward_view, what plane_median_gradients
    was handed and the view's gradients after it."""

    def __init__(self, base, T, run, monkeypatch):
        self.base = base
        gsr = T.gsr
        inv_depth_of = sub("_frame").inv_depth_of
        of_frame = lambda buffers: next((c for c in reversed(base.calls) if c["frame_buf"] is buffers), None)
        render, backward = gsr.render_view, gsr.backward_view
        median, plane, plane_median = (gsr.median_depth.render_median_depth, gsr.plane_depth.render_view_plane_depth,
                                       gsr.plane_depth.render_view_plane_median_depth)
        pm_gradients = gsr.plane_depth.plane_median_gradients
        clone = lambda t: None if t is None else t.clone()

        def render_view(params, camera, background, **kw):
            n = len(base.calls)
            out = render(params, camera, background, **kw)
            if len(base.calls) > n:
                base.calls[-1]["invd"] = inv_depth_of(out[2], int(params["positions"].shape[0]), out[0].device).clone()
            return out

        def render_median_depth(buffers, *args, **kw):
            out = median(buffers, *args, **kw)
            call = of_frame(buffers)
            if call is not None:
                call.update(depth_img=out[0].clone(), contrib=out[1].clone())
            return out

        def render_view_plane_depth(params, camera, buffers):
            out = plane(params, camera, buffers)
            call = of_frame(buffers)
            if call is not None:
                call.update(depth_img=out[0].clone(), slopes=out[1].clone(), normals=out[2].clone())
            return out

        def render_view_plane_median_depth(params, camera, buffers):
            out = plane_median(params, camera, buffers)
            call = of_frame(buffers)
            if call is not None:
                call.update(depth_img=out[0].clone(), contrib=out[1].clone(), slopes=out[2].clone(), normals=out[3].clone())
            return out

        def backward_view(params, camera, background, buffers, dL_dpixels, **kw):
            call = of_frame(buffers)
            if call is not None:
                call["new_kw"] = {k: clone(kw[k]) for k in NEW_KW if kw.get(k) is not None}
            g = backward(params, camera, background, buffers, dL_dpixels, **kw)
            if call is not None:
                call["view_grads"] = g                                                # (the dict train_view goes on with)
            return g

        def plane_median_gradients(params, camera, buffers, dL_dmedian, contrib, slopes, normals, grads=None):
            call = of_frame(buffers)
            if call is not None:
                call["pm_args"] = {"g": dL_dmedian.clone(), "contrib": contrib.clone(), "slopes": slopes.clone(), "normals": normals.clone(),
                                   "into_grads": grads is not None}
            out = pm_gradients(params, camera, buffers, dL_dmedian, contrib, slopes, normals, grads=grads)
            if call is not None:                                                       # the view's gradients, whatever the call was handed
                call["out_after"] = {k: call["view_grads"][k].clone() for k in base.OUT if call["view_grads"].get(k) is not None}
            return out

        monkeypatch.setattr(gsr, "render_view", render_view)
        monkeypatch.setattr(gsr, "backward_view", backward_view)
        monkeypatch.setattr(gsr.median_depth, "render_median_depth", render_median_depth)
        monkeypatch.setattr(gsr.plane_depth, "render_view_plane_depth", render_view_plane_depth)
        monkeypatch.setattr(gsr.plane_depth, "render_view_plane_median_depth", render_view_plane_median_depth)
        monkeypatch.setattr(gsr.plane_depth, "plane_median_gradients", plane_median_gradients)

    def take(self):
        """The base recorder's calls since the last take(), each with this recorder's captures as numpy."""
        torch.cuda.synchronize()
        mine = []
        for c in self.base.calls:
            d = {k: to_np(c.get(k)) for k in ("invd", "depth_img", "contrib", "slopes", "normals")}
            d["new_kw"] = {k: to_np(t) for k, t in c.get("new_kw", {}).items()}
            d["pm_args"] = None if c.get("pm_args") is None else {k: (to_np(t) if torch.is_tensor(t) else t) for k, t in c["pm_args"].items()}
            d["out_after"] = None if c.get("out_after") is None else {k: to_np(t) for k, t in c["out_after"].items()}
            mine.append(d)
        calls = self.base.take()
        for call, d in zip(calls, mine):
            call.update(d)
        return calls


def begin(name, monkeypatch, argv=None):
    T, run, base = start(CONFIGS[name] if argv is None else argv, monkeypatch, prepare)
    return T, run, DepthRecorder(base, T, run, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------- the checks
def check_depth_frame(dmode, call, fr, worst):
    """The contributor and the mode's image against what the kernel tests hold.  Returns median_f64 of the frame (None under plane,
    whose image check needs the yardstick: check_plane_image)."""
    if dmode == "plane":
        return None
    ref = M.median_f64(fr)
    share = float(ref["tie"].mean())
    keep(worst, "frame/tie_share", share / M.MAX_TIES)
    assert share <= M.MAX_TIES, share
    contrib, img = call["contrib"].astype(np.int64), call["depth_img"]
    assert np.array_equal(contrib[~ref["tie"]], ref["contrib"][~ref["tie"]]), "the contributor is not the float64 median outside the tie mask"
    if dmode == "median":
        ids = DS.chosen_ids(fr, contrib)
        want = np.where(ids >= 0, fr["invd"][np.maximum(ids, 0)], np.float32(0)).astype(np.float32)
    else:
        want = PM.chosen(fr, call["slopes"], contrib)["m"]
    assert img.tobytes() == want.tobytes(), "the mode's depth image is not the named entry's value bit for bit"
    assert ((contrib > 0) == (DS.chosen_ids(fr, contrib) >= 0)).all()
    return ref


def check_slopes(call, snap, filt, worst):
    """The captured slopes -- what the render and, through their (0, 0) pattern, the float64 side's branch read -- against
    plane_depth_reference.slopes_f32 of the RAW scales of the parameters and the captured normals (tests/test_gpu_plane_depth.py's
    criterion: the same branch, values within 8 eps32 of the largest), Gaussians with a step-5 decision within
    plane_depth_reference.MARGIN_CAP of its threshold aside.  Under the filter the Gaussians that are flat by their raw scales and
    round by their filtered ones must be among those compared, and carry slopes wherever the raw scales say they do."""
    cam, P = call["cam"], snap["P"]
    n = int(np.asarray(P["positions"]).reshape(-1, 3).shape[0])
    raw, pos = np.asarray(P["scales"], np.float32).reshape(n, 3), np.asarray(P["positions"], np.float32).reshape(n, 3)
    view = np.asarray(cam["world_to_camera"], np.float32).reshape(4, 4)
    H, W = call["dep"].shape
    want, fallback = PD.slopes_f32(call["normals"], raw, pos, view, cam["tan_fovx"], cam["tan_fovy"], W, H)
    far = PD.branch_margins(call["normals"], raw, pos, view) > PD.MARGIN_CAP
    got = call["slopes"]
    keep(worst, "frame/slopes_near", float((~far).mean()) / 0.01)
    assert (~far).mean() <= 0.01, "too many Gaussians near a branch threshold"
    assert np.array_equal((got != 0).any(1)[far], ~fallback[far]), "a Gaussian's branch is not that of its raw scales"
    e = float(np.abs(got.astype(np.float64) - want)[far].max() / (8.0 * PD.EPS32 * np.abs(want).max()))
    keep(worst, "frame/slopes", e)
    assert e <= 1.0 and (~fallback).mean() > 0.5, (e, float((~fallback).mean()))
    if filt is not None:
        flat = lambda s: np.sort(s, 1)[:, 0] <= PD.MAX_FLATNESS * np.sort(s, 1)[:, 1]
        turned = flat(raw) & ~flat(np.asarray(S.scene_of(P, filt)["scales"], np.float32)) & far
        live = turned & ~fallback
        print(f"    view {call['v']}: {int(turned.sum())} Gaussians flat raw and round filtered, {int(live.sum())} of them on the plane branch")
        assert live.sum() >= MIN_FLAT_TO_ROUND and (got[live] != 0).any(1).all()


def check_plane_image(call, fr, r, worst):
    """The plane image within 3 E_f32 + eps32 of plane_depth_reference.yardstick, E_f32 the restatement's error on this frame
    (tests/test_gpu_plane_depth.py's forward criterion)."""
    E_k = PD.image_error(call["depth_img"], r, fr["invd"])
    E_32 = PD.image_error(PD.render_f32(fr, call["slopes"])[0], r, fr["invd"])
    bound = 3.0 * E_32 + PD.EPS32
    print(f"    view {call['v']}: plane image error {E_k:.3e} (float32 restatement {E_32:.3e}), {int(r['mask'].sum())} pixels masked")
    keep(worst, "frame/plane_image", E_k / bound)
    keep(worst, "frame/plane_masked", float(r["mask"].mean()) / DS.MAX_MASKED)
    assert E_k <= bound and r["mask"].mean() <= DS.MAX_MASKED, (E_k, E_32)


def compare(worst, key, got, want, bound, keep_pixels=None, who=""):
    e = np.abs(np.asarray(got, np.float64).reshape(np.shape(want)) - want)
    e = float((e if keep_pixels is None else e[keep_pixels]).max())
    print(f"    {who}{key} err {e:.3e} (bound {bound:.3e}, max {np.abs(want).max():.3e})")
    keep(worst, "image/" + key, e / bound if bound > 0 else float(e > 0))
    assert e <= bound, (key, e, bound)


def check_image_half(dmode, run, call, worst, it, alive):
    """The trainer's cotangent images against depth_step_reference.image_half, and the keywords that reached backward_view."""
    v = call["v"]
    H, W = call["dep"].shape
    tg, cfg = targets_of(run, v, None, it)
    frame = {"img": call["img"], "dinv": call["dep"], "final_T": call["buf"]["final_Ts"], "cam": call["cam"], "nimg": call["nimg"],
             "depth_img": call["depth_img"], "contrib": call["contrib"]}
    res = DS.image_half(dmode, frame, tg, cfg)
    bounds = DS.image_half_bounds(dmode, res, tg, cfg)
    who = f"view {v}: "
    # the keywords: exactly the mode's, and the consistency term's three exactly when the statement has the term
    assert sorted(call["new_kw"]) == KW_OF[dmode], (dmode, sorted(call["new_kw"]))
    want_kw = ["dL_dnormal_image", "gaussian_normals", "normal_image"] if res["gN"] is not None else (["gaussian_normals"] if dmode == "plane" else [])
    assert call["term_kw"] == want_kw, (call["term_kw"], want_kw)
    if dmode == "median":
        assert np.array_equal(call["new_kw"]["median_contributor"].reshape(H, W), call["contrib"])
        got = call["new_kw"]["dL_dmedian_depth"]
    elif dmode == "plane":
        assert call["new_kw"]["plane_depth_image"].tobytes() == call["depth_img"].tobytes()
        assert call["new_kw"]["plane_slopes"].tobytes() == call["slopes"].tobytes() and call["normals32"].tobytes() == call["normals"].tobytes()
        got = call["new_kw"]["dL_dplane_depth"]
    else:
        pm = call["pm_args"]
        assert pm is not None, "plane_median_gradients was not called on this frame"
        assert np.array_equal(pm["contrib"], call["contrib"]) and pm["slopes"].tobytes() == call["slopes"].tobytes()
        assert pm["normals"].tobytes() == call["normals"].tobytes()
        got = pm["g"]
    call["g_term"] = np.asarray(got, np.float32).reshape(H, W)
    ties = float(res["ties"].mean())
    keep(worst, "image/sign_ties", ties / DS.MAX_SIGN_TIES)
    assert ties <= DS.MAX_SIGN_TIES
    assert np.abs(res["g_term"]).max() > 0 or not alive
    compare(worst, "g_term", call["g_term"], res["g_term"], bounds["g_term"], ~res["ties"], who)
    if dmode != "plane":                                                    # outside the mask the kernel writes exact zeros
        assert not call["g_term"][res["mask"] == 0].any()
    pix = S.tie_pixels(call["img"], None, tg["target"])
    assert pix.mean() <= 1e-3
    compare(worst, "dpix", call["dpix"], res["dpix"], bounds["dpix"], ~pix, who)
    for k in ("gD", "gA"):
        assert (call[k] is None) == (res[k] is None), (k, "present" if call[k] is not None else "absent")
        if res[k] is not None:
            assert np.abs(res[k]).max() > 0 or not alive, k
            compare(worst, k, call[k], res[k], bounds[k], None, who)
    if res["gN"] is not None:
        far = ~res["near"]
        assert res["near"].mean() <= 1e-2 and not call["gN"][far & ~res["counted"]].any()
        compare(worst, "gN", call["gN"], res["gN"], bounds["gN"], far, who)
    return res, tg


def check_plane_median_adds(before, after):
    """After plane_median_gradients: every key but the two it adds into keeps the bits backward_view returned, and those two moved."""
    assert set(after) == set(before)
    for k in before:
        if k in ("dL_dmean3D", "dL_drot"):
            assert not np.array_equal(after[k], before[k]), k
        else:
            assert after[k].tobytes() == before[k].tobytes(), k


@pytest.mark.parametrize("name", list(CONFIGS))
def test_depth_terms_in_a_train_step_against_float64(name, monkeypatch):
    T, run, rec = begin(name, monkeypatch)
    a = run.args
    dmode, mode, dense, worst = a.depth_render, a.rasterize_mode, a.dense_sh, {}
    seen = np.zeros(run.model.num_points, np.int64)
    grads0 = None
    for it in range(a.iterations):
        snap = snapshot(run)
        T.train_step(run, it)
        calls = rec.take()
        overflowed = {(r["iteration"], r["view"]) for r in run.capacity_log}
        print(f"\n{name} iteration {it}: views {[c['v'] for c in calls]}" + (f", overflowed {sorted(overflowed)}" if overflowed else ""))
        views64, batch, first = [], [], set()
        for call in calls:
            v = call["v"]
            if (it, v) in overflowed and v not in first:                    # the overflowed frame: nothing of it is trusted, or used
                first.add(v)
                assert call["capacity"] is not None
                continue
            filt, cam = snap["filter"], call["cam"]
            H, W = call["dep"].shape
            pre = S.preprocess(snap["P"], cam, mode, filt)
            check_frame(call, pre, mode, filt is not None, worst)
            normals = check_term_frame(call, snap, pre, mode, worst)
            if normals is None and dmode != "median":
                normals, _ = S.gaussian_normals_f64(snap["P"], cam, captured=call["normals"])
            if dmode != "median":
                check_slopes(call, snap, filt, worst)
            fr = DS.frame_of(call["buf"], W, H, call["invd"])
            ref = check_depth_frame(dmode, call, fr, worst)
            res, tg = check_image_half(dmode, run, call, worst, it, alive=it == 0)
            before = call["out"]
            if dmode == "plane-median":                                     # the gradients after the term's last writer
                assert call["out_after"] is not None
                call["out"] = call["out_after"]
            rest = S.param_half(snap["P"], cam, call["buf"]["point_list"], call["buf"]["ranges"], call["dpix"], call["gD"], call["gA"],
                                rasterize_mode=mode, filter_3d=filt, pre=pre, gN=call["gN"], normals=normals if call["gN"] is not None else None)
            term = DS.term_gradients(dmode, snap["P"], cam, pre, fr, call["g_term"], call["contrib"], call["slopes"], normals, filter_3d=filt,
                                     nb=call["buf"], image=call["depth_img"])
            if dmode == "plane":
                check_plane_image(call, fr, term["yardstick"], worst)
            v64 = DS.view_gradients(rest, term)
            check_view_gradients(call, v64, dense, worst)
            if dmode == "plane-median":
                check_plane_median_adds(before, call["out"])
            if it == 0:                                                     # (iteration 1 follows the opacity reset: nothing crosses one half)
                share = DS.term_share(v64)
                print(f"    view {v}: the term's share of sum|g| " + ", ".join(f"{k} {x:.2f}" for k, x in share.items()))
                for k in ("dL_dmean3D",) + (() if dmode == "median" else ("dL_drot",)):
                    keep(worst, "share/" + k, MIN_SHARE / max(share.get(k, 0.0), 1e-300))
                    assert share.get(k, 0.0) >= MIN_SHARE, (k, share)
                if dmode != "plane":
                    cond = DS.conditions(dmode, fr, call["contrib"], tg, ref, call["slopes"])
                    print(f"    view {v}: {cond}")
                    DS.assert_conditions(dmode, cond, f"{name} view {v}", view=v)
            views64.append(v64)
            batch.append(v)
            seen += call["buf"]["radii"] > 0
        assert len(batch) == a.views_per_step == len(set(batch))
        if it == 0:                                                         # (what the CPU test settled its conditions for)
            assert tuple(batch) == FIRST_VIEWS[name], (batch, FIRST_VIEWS[name])
            if snap["filter"] is not None:
                assert DS.flat_raw_round_filtered(snap["P"], snap["filter"]) >= MIN_FLAT_TO_ROUND
        G64 = DS.step_gradient(views64, len(batch), snap["P"]["positions"], sh="dense" if dense else "payloads")
        for k in A.GROUPS:
            if k != "shs" or dense:
                grad_ratios(worst, "batch/" + k, to_np(run.model.grads[k]), G64[k])
        if it == 0:
            grads0 = {k: to_np(run.model.grads[k]).astype(np.float64) for k in S.SMALL}
            if name in ("D1", "D2"):
                # (on this scene 2 % of the live SH elements lie between the kernel check's 1e-6 and the sign step's exact 1.09e-6)
                check_adam(run, rec.base.after_adam, snap, G64, {k: s.get_lr(0, a.iterations) for k, s in run.sched.items()}, worst,
                           sign_step_min=100.0 * (A._f(1e-8) + A.DIV_EPS))
        if run.screen_stats:
            assert np.array_equal(to_np(run.model.stats.vis_count), seen), "vis_count is not the number of batch views that saw each Gaussian"
    worst = {f"{name}/{k}": v for k, v in worst.items()}
    if name == "D6":                                                        # without an overflow the configuration proves nothing
        assert run.capacity_log and (run.capacity_log[0]["iteration"], run.capacity_log[0]["capacity"]) == (0, 64)
        assert all(r["D"] > r["capacity"] for r in run.capacity_log)
    if name == "D8":
        assert run.screen_stats
    if name in SERIAL:                                                      # the path against the serial, sized run of the same parameters
        r_serial, serial = first_step_grads(SERIAL[name], monkeypatch, prepare)
        assert not r_serial.capacity_log
        spread(worst, f"paths/{name}", grads0, serial)
    settle(worst, MARGINS, NOTE)
