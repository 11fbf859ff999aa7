#!/usr/bin/env python3
"""
Counterpart of the reference's training iteration (train.py:920-1066) on the
MI355X: per step each rank renders its views, forms the L1 loss and pixel gradient, runs backward, all-reduces
the gradient (11 floats all-reduced + 3 floats all-gathered per Gaussian, the SH gradient rebuilt per rank: dist.py), and applies the fused Adam update -- everything on the GPU,
parameters resident, no per-iteration host upload.  Then the reference's adaptive density control (row f4,
train.py:351-713: clone / split / prune / opacity reset) runs on the replicated parameters -- it is deterministic,
so every rank reaches the same point set without a collective -- and rank 0 writes PLY checkpoints (train.py:796-803).

Targets: with --dataset <NeRF-synthetic dir> the train split (transforms_train.json + PNGs, alpha dropped as
train.py:323-334) is used; without it, targets are renders of a hidden seeded scene from orbiting cameras.

    python examples/train.py --iterations 200 --gaussians 20000
    python examples/train.py --gpus 8 --views-per-step 8        (launches its own 8 ranks; or under torch.distributed.run)

Depth and alpha supervision (include/gsr_aux_grads.h): --lambda-depth adds lambda_d times the masked L1 of the rendered inverse
depth (targets: --depth-dir with --dataset, one float32 (H, W) .npy per frame named after its file_path; else the hidden scene's own
inverse depth; mask = target > 0), --lambda-alpha lambda_a times the L1 of the alpha image 1 - final_T (targets: the PNG alpha,
or the hidden scene's).  Both terms are normalised by W H, as the reference's depth_loss.  That L1 needs targets in the scene's own
units.  --depth-loss pearson (include/gsr_depth_corr.h) is for relative targets instead -- inverse depth known only up to an unknown
scale a > 0 and shift b per image, t -> a t + b, as a monocular depth network gives it: the depth term is then lambda_d times
1 - the Pearson correlation of the rendered inverse depth with the target over the same mask, which no such a and b change (it is
O(1) already: no W H).  For experiments, --depth-noise S (seed --depth-seed) stores every view's depth target as a_v t + b_v on its
masked pixels, a_v = exp(U(-S, S)), b_v = U(0, S) times the view's mean target; the summary then scores the depth against the
clean targets too (train_depth_l1_clean_mean), and always reports the mean correlation and each view's fitted (s, b).

A normal prior (include/gsr_normals.h): --lambda-normal adds lambda_n times the cosine loss 1 - n . t between the normals of the
rendered depth (the unit cross product of the central differences of the camera-space points, where the pixel's and its four
neighbours' alpha reaches --normal-alpha-min) and normal targets, normalised by W H; its two gradient images are added to those of
the depth and alpha terms.  Targets: --normal-dir with --dataset, one float32 (H, W, 3) .npy per frame named after its file_path, in
camera space (x right, y down, z forward: normals that face the camera have z < 0) or, with --normal-space world, in world space;
else the normals of the hidden scene's own depth.  --normal-noise S (seed --normal-seed) adds N(0, S^2) to every component of every
target once at load, for experiments.  The summary reports the mean angle between the depth normals and the clean targets
(train_normal_angle_deg_mean) and the share of pixels that have a depth normal (train_normal_valid_share).

Depth distortion (include/gsr_distortion.h, distortion.py): --lambda-dist W adds W times the mean over the pixels of
Dist(p) = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2, m the inverse view depth -- the regulariser the surface methods (2DGS, GOF, PGSR,
RaDe-GS) train with before they extract a mesh: it pulls the Gaussians along a ray onto one surface.  It needs no target.
--dist-from-iter K switches it on at iteration K (the methods above start it once the colours have settled).  With the weight, or
with --report-distortion alone, the summary has train_distortion_mean: the mean of Dist over pixels and views at the end.

Normal consistency (include/gsr_normal_render.h, normal_render.py): --lambda-normal-consistency W adds W times the mean over the
pixels of 1 - n_d . N / |N|, N the blended image of the Gaussians' own normals (each the direction of its Gaussian's shortest axis,
facing the camera) and n_d the normals of the rendered depth -- the second geometric term of the same methods, which turns the
Gaussians the distortion term flattened into the surface.  No target is needed; the gradient goes to both sides.
--normal-consistency-from-iter K switches it on at iteration K.  With the weight, or with --report-normal-consistency alone, the
summary has train_normal_consistency_deg: the mean angle in degrees between N / |N| and n_d over counted pixels and views at the end.

Median depth (include/gsr_median_depth.h, median_depth.py): --depth-render median takes --lambda-depth's L1 on the median inverse depth
(the inverse depth of the Gaussian at which the transmittance falls through one half) instead of the expected inverse depth, masked
to the target's mask and to the pixels that have a median; its gradient reaches only the chosen Gaussian's depth, through a stage of
the backward.  The summary then has train_median_depth_l1_mean beside train_depth_l1_mean.  --mesh-depth median makes --mesh-out fuse
the median depth.  Both default to "expected": today's behaviour.

Plane depth (include/gsr_plane_depth.h, plane_depth.py): --depth-render plane takes --lambda-depth's L1 on the blended ray-plane
intersection inverse depth -- each flat Gaussian contributes the depth at which the pixel's ray meets its plane, not its centre's -- and,
with --lambda-normal-consistency, takes that term's depth normals from it too; the gradient reaches positions, rotations, shapes and
opacities through a stage of the backward.  The summary then has train_plane_depth_l1_mean.  --mesh-depth plane makes --mesh-out fuse
the plane depth.

Plane depth under the median rule (include/gsr_plane_median.h, plane_depth.py): --depth-render plane-median takes --lambda-depth's L1 on
the inverse depth at which the pixel's ray meets the plane of the ONE Gaussian at which the transmittance falls through one half (what
RaDe-GS and GOF fuse), masked like --depth-render median.  Its gradient reaches that Gaussian's position and rotation and needs no
stage of the backward: plane_depth.plane_median_gradients adds it to the view's gradients after backward_view.  The summary then has
train_plane_median_depth_l1_mean.  --mesh-depth plane-median makes --mesh-out fuse that depth.

Pose refinement (include/gsr_camera_grads.h, pose.py): --optimize-poses keeps a pose correction xi = (rho, phi) per view and
trains it with Adam (--pose-lr) on backward(camera_grad=True)'s camera gradients beside the Gaussians; each step reads that view's
35 camera floats back to the host (one wait per view and iteration).  --pose-noise-deg / --pose-noise-trans (seed --pose-seed)
perturb the dataset poses first, for experiments; the --log summary then records the per-view pose error against the dataset
poses (degrees, scene units) at the start and the end.  One GPU only.

Density control on screen-space statistics (include/gsr_densify_stats.h): --densify-stat screen accumulates, per Gaussian, the norm
of dL/dmean2D over every view that saw it since the last density-control call (one small kernel after each view's backward, on that
view's stream), marks clone / split candidates from the average against --densify-grad-threshold, and prunes also by
--prune-screen-size (pixels) and --prune-world-size (fraction of the scene extent) once past the first opacity reset.  --absgrad
accumulates the sums of per-pixel magnitudes instead (AbsGS; thresholds of 2-4x the signed one are usual).  The default,
--densify-stat reference, is the reference trainer's rule: the 3D position gradient of the last view.

3D smoothing filter (include/gsr_filter3d.h, filter3d.py): --filter-3d trains under Mip-Splatting's 3D filter, the other half of
--rasterize-mode antialiased; --eval-scales 1,2,4,8 scores the result at lower resolutions, where the two matter.

Exposure compensation (include/gsr_exposure.h, exposure.py): --optimize-exposure keeps an affine colour transform E_v per training
view (12 numbers, c' = c A + b) and trains it with Adam (--exposure-lr-init -> --exposure-lr-final) beside the Gaussians: the loss sees
the corrected render, and the step stays free of host waits.  --exposure-noise S (seed --exposure-seed) perturbs every training target
once at load, for experiments.  Training views are then scored through their learned E_v, held-out views with the identity; the
matrices go to the summary and to exposure.json beside each PLY.  One GPU only, and not with --capacity.

Per-pixel loss weights (include/gsr_weighted_loss.h, loss.PixelWeights): --mask-dir DIR reads <DIR>/<basename of file_path>.png
per training view, first channel / 255 = the weight of that pixel in the colour loss (0 = ignore: a passer-by, a shadow, sky), for
L1 alone and with --lambda-dssim, also under --optimize-exposure.  --mask-dilate R (default 5, the SSIM window's radius) first grows
the ignored region by R pixels: only then is what it covers invisible to the SSIM term too.  The loss curve is normalised per view
by 3 M_v, M_v the view's weight total; the summary adds the weighted L1 / PSNR / SSIM beside the plain ones.  For experiments,
--occluders K (--occluder-seed, --occluder-size F) pastes K opaque saturated rectangles of side up to F of the image's into every
training target at load, elsewhere in every view; --mask-occluders trains with the masks of exactly those rectangles, dilated, and
the summary then also scores every view against the clean targets (clean_psnr_mean, clean_ssim_mean, clean_l1_mean).

Starting from a point cloud (include/gsr_knn.h, knn.py): --init knn keeps the reference start's positions and gives every Gaussian
the isotropic scale the original 3DGS starts with, the root of the mean squared distance to its three nearest neighbours, instead
of the constant 0.1; --init-points FILE.ply starts from the points (and uchar colours) of a binary PLY the same way
(point_cloud.gaussians_from_points) and takes the point count from the file.  The --log header records `init`, the smallest, median and
largest initial scale, and `first_iteration_pairs`, the (tile, Gaussian) pair count D of the run's first frame.

A mesh of the result (include/gsr_tsdf.h, tsdf.py): --mesh-out FILE.ply renders depth and colour from the training views after the
last iteration, fuses them into a TSDF volume of --mesh-resolution voxels per side (default 256) and writes the marching-tetrahedra
mesh of the cells observed with weight --mesh-min-weight; the function examples/extract_mesh.py runs on a checkpoint.  Off by
default; nothing changes when it is off.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# before torch / the HIP runtime load: dmabuf IPC is what this pool's driver supports, and a rank started by torch.distributed.run
# (not by launch.py) would otherwise never get it
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


# flags whose state one rank owns: refused before the ranks start (_self_launch) and again, with the world size known, in check_args
ONE_GPU_ONLY = {
    "optimize_poses": "--optimize-poses trains on one GPU only (per-rank pose ownership is not implemented): drop --gpus",
    "optimize_exposure": "--optimize-exposure trains on one GPU only (per-rank exposure ownership is not implemented): drop --gpus"}


def refuse(rules):
    """rules: (violated, message) in the order that decides which message a doubly wrong command line gets"""
    for violated, message in rules:
        if violated:
            raise SystemExit(message)


def _self_launch():
    """`python examples/train.py --gpus N` (no WORLD_SIZE): start the N ranks before anything here touches the GPU."""
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--optimize-poses", action="store_true")
    ap.add_argument("--optimize-exposure", action="store_true")
    known = ap.parse_known_args()[0]
    gpus = known.gpus
    refuse((gpus > 1 and getattr(known, flag), ONE_GPU_ONLY[flag]) for flag in ("optimize_exposure", "optimize_poses"))
    if gpus > 1 and "WORLD_SIZE" not in os.environ:
        from importlib import util as _ilu
        spec = _ilu.spec_from_file_location("gsr_launch", os.path.join(ROOT, "3dgs-native_amd", "launch.py"))
        launch = _ilu.module_from_spec(spec)
        spec.loader.exec_module(launch)
        rc = launch.launch_ranks(os.path.abspath(__file__), sys.argv[1:], gpus)
        sys.exit(rc if rc >= 0 else 128 - rc)


if __name__ == "__main__":
    _self_launch()

import time  # noqa: E402
from types import SimpleNamespace  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

gsr = importlib.import_module("3dgs-native_amd")


def load_nerf(path, max_views, split="train", alpha=False, depth_dir=None):
    """(cams, targets), and with alpha=True also the PNGs' alpha channels / 255 as (H, W) float32 (ones for a PNG without one);
    with depth_dir also the inverse-depth targets, <depth_dir>/<basename of file_path>.npy."""
    from PIL import Image
    angle, frames = gsr.cameras.nerf_frames(path, max_views, split)
    cams, targets, alphas, depths = [], [], [], []
    for file_path, png, name, pose in frames:
        img = np.asarray(Image.open(png), dtype=np.float32) / 255.0
        targets.append(img[:, :, :3].copy())
        alphas.append(img[:, :, 3].copy() if img.ndim == 3 and img.shape[2] == 4 else np.ones(img.shape[:2], np.float32))
        if depth_dir is not None:
            d = np.load(os.path.join(depth_dir, name + ".npy")).astype(np.float32)
            if d.shape != img.shape[:2]:
                raise ValueError(f"{file_path}: depth target {d.shape} for a {img.shape[:2]} image")
            depths.append(d)
        cams.append(gsr.cameras.nerf_camera(pose, img.shape[1], img.shape[0], angle))
    out = (cams, targets) + ((alphas,) if alpha else ()) + ((depths,) if depth_dir is not None else ())
    return out


def load_normals(path, normal_dir, max_views, shapes, split="train"):
    """The normal targets of --normal-dir: <normal_dir>/<basename of file_path>.npy per frame, float32 (H, W, 3), any length (a zero
    vector: the pixel has no target)."""
    out = []
    for (file_path, _, name, _), hw in zip(gsr.cameras.nerf_frames(path, max_views, split)[1], shapes):
        n = np.load(os.path.join(normal_dir, name + ".npy")).astype(np.float32)
        if n.shape != tuple(hw) + (3,):
            raise ValueError(f"{file_path}: normal target {n.shape} for a {tuple(hw)} image")
        out.append(n)
    return out


def load_masks(path, mask_dir, max_views, shapes, split="train"):
    """The weight images of --mask-dir: <mask_dir>/<basename of file_path>.png per frame, first channel / 255, (H, W) float32; its
    shape must be its image's."""
    from PIL import Image
    masks = []
    for (file_path, _, name, _), shape in zip(gsr.cameras.nerf_frames(path, max_views, split)[1], shapes):
        png = np.asarray(Image.open(os.path.join(mask_dir, name + ".png")))
        m = (png if png.ndim == 2 else png[:, :, 0]).astype(np.float32) / 255.0
        if m.shape != tuple(shape):
            raise ValueError(f"{file_path}: mask {m.shape} for a {tuple(shape)} image")
        masks.append(np.ascontiguousarray(m))
    return masks


def occluder_rects(H, W, count, size, seed, view):
    """--occluders: `count` rectangles (y0, y1, x0, x1, rgb) for one view -- sides between 0.3 and 1 times `size` of the image's
    side, anywhere inside the image, a saturated colour each (one channel 1, one 0, one random); seeded by (seed, view)."""
    rng = np.random.default_rng([seed, view])
    rects = []
    for _ in range(count):
        h, w = (max(1, int(rng.uniform(0.3, 1.0) * size * n)) for n in (H, W))
        y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        rgb = np.zeros(3, np.float32)
        hi, lo, mid = rng.permutation(3)
        rgb[hi], rgb[mid] = 1.0, rng.random()
        rects.append((y0, y0 + h, x0, x0 + w, rgb))
    return rects


def paste_occluders(target, rects):
    """(the (H, W, 3) numpy target with the rectangles pasted, their mask: 0 on a rectangle, 1 elsewhere)"""
    out, mask = target.copy(), np.ones(target.shape[:2], np.float32)
    for y0, y1, x0, x1, rgb in rects:
        out[y0:y1, x0:x1] = rgb
        mask[y0:y1, x0:x1] = 0.0
    return out, mask


def mode_keywords(args):
    """What every render and backward of a run is given beside its view (run.mode_kw): --rasterize-mode antialiased's keyword;
    --filter-3d adds {"filter_3d": the current filter} at every recompute_filter()."""
    return {"rasterize_mode": args.rasterize_mode} if args.rasterize_mode != "classic" else {}


def parse_eval_scales(text, W, H):
    """--eval-scales "1,2,4": integers >= 1 that divide W and H (the target is box-averaged by s x s)."""
    if not text:
        return []
    try:
        scales = [int(x) for x in text.split(",")]
    except ValueError:
        raise SystemExit(f"--eval-scales takes integers separated by commas (got {text!r})") from None
    for sc in scales:
        if sc < 1 or W % sc or H % sc:
            raise SystemExit(f"--eval-scales: {sc} does not divide the {W} x {H} image")
    return scales


def row_mean(rows, key):
    return float(np.mean([r[key] for r in rows]))


def row_means(rows, prefix):
    """{"<prefix>_l1_mean", "<prefix>_psnr_mean", "<prefix>_ssim_mean"} of score_views' rows"""
    return {f"{prefix}_{k}_mean": row_mean(rows, k) for k in ("l1", "psnr", "ssim")}


def score_scales(P, cams, targets, bg, mode_kw, scales, exposure=None):
    """{s: {"psnr", "ssim"}}: every view also rendered at W/s x H/s with the same field of view, against its target box-averaged by
    s x s (what a camera s times as far away, or a zoom-out by s, would record)."""
    out = {}
    for sc in scales:
        small = [dict(c, width=c["width"] // sc, height=c["height"] // sc) for c in cams]
        tg = [t.reshape(c["height"] // sc, sc, c["width"] // sc, sc, 3).mean((1, 3)).contiguous() for c, t in zip(cams, targets)]
        rows, _ = score_views(P, small, tg, bg, mode_kw, exposure)
        out[str(sc)] = {"psnr": row_mean(rows, "psnr"), "ssim": row_mean(rows, "ssim")}
    return out


def score_views(P, cams, targets, bg, mode_kw, exposure=None):
    """Per-view mean L1, PSNR (10 log10(1 / MSE), colours in [0, 1]) and SSIM (gaussian window, gsr_loss.h) of the current model;
    the images come back too.  `exposure` (an ExposureModel whose rows are these views): view k is scored through its E_k."""
    rows, images = [], []
    for k, (c, t) in enumerate(zip(cams, targets)):
        img = gsr.render_view(P, c, bg, **mode_kw)[0].reshape(t.shape)
        if exposure is not None:
            img = gsr.exposure.apply_exposure(img, exposure.matrix(k), out=img)
        d = img - t
        mse = float((d * d).mean().item())
        rows.append({"l1": float(d.abs().mean().item()), "psnr": (10.0 * np.log10(1.0 / mse)) if mse > 0 else float("inf"),
                     "ssim": gsr.loss.ssim(img, t, window="gaussian")})
        images.append(img)
    return rows, images


def weighted_scores(img, t, w):
    """score_views' three numbers under a PixelWeights w: sum m |d| / (3 M), PSNR of sum m d^2 / (3 M), and ssim_sum / M"""
    M = float(w.total.item())
    l1_sum, ssim_sum, _ = gsr.loss.l1_dssim_loss_and_gradients(img, t, 0.0, window="gaussian", want_grad=False, weights=w)
    d = img - t
    mse = float((w.weights[..., None] * d * d).sum().item()) / (3.0 * M)
    return {"l1": float(l1_sum.item()) / (3.0 * M), "psnr": (10.0 * np.log10(1.0 / mse)) if mse > 0 else float("inf"),
            "ssim": float(ssim_sum.item()) / M}


def perturb_depth_targets(depth_targets, noise, seed):
    """--depth-noise S: every view's target as a relative depth source would store it, a_v t + b_v on the masked pixels (t > 0, taken
    from the clean target: a_v > 0 and b_v >= 0 keep it) with a_v = exp(U(-S, S)) and b_v = U(0, S) * mean(t over the mask)."""
    rng = np.random.default_rng(seed)
    out = []
    for t in depth_targets:
        a, u = float(np.exp(rng.uniform(-noise, noise))), float(rng.uniform(0.0, noise))
        mask = t > 0
        b = u * float(t[mask].mean().item()) if bool(mask.any().item()) else 0.0
        out.append(torch.where(mask, a * t + b, t).contiguous())
    return out


def aux_scores(P, cams, depth_targets, alpha_targets, bg, mode_kw, clean_depth_targets=None, median=False, plane=False, plane_median=False):
    """Mean masked inverse-depth L1 (sum |D - t| [t > 0] / (W H), as depth_loss) and mean alpha L1 over the views; None without targets.
    Third: with depth targets, {"train_depth_corr_mean": the mean Pearson correlation rho of the rendered inverse depth with the
    targets as given, "train_depth_fit": each view's (s, b) of render ~ s target + b (include/gsr_depth_corr.h)}, and with
    clean_depth_targets (--depth-noise) "train_depth_l1_clean_mean", the first score against the unperturbed targets; with `median`
    (--depth-render median) "train_median_depth_l1_mean", the first score of the median inverse depth over the pixels that have one;
    with `plane` (--depth-render plane) "train_plane_depth_l1_mean", the first score of the plane-depth image; with `plane_median`
    (--depth-render plane-median) "train_plane_median_depth_l1_mean", the first score of the plane depth under the median rule over the
    pixels that have one."""
    dl, al, dc, dm, dp, dpm = [], [], [], [], [], []
    fits = torch.zeros((len(cams), 4), device=P["positions"].device) if depth_targets is not None else None
    for k, c in enumerate(cams):
        _, dep, buf = gsr.render_view(P, c, bg, **mode_kw)
        if depth_targets is not None:
            t = depth_targets[k]
            dl.append(float(gsr.loss.depth_loss_and_gradients(dep, t, (t > 0).float(), want_grad=False)[0].item()) / t.numel())
            gsr.loss.depth_corr_loss_and_gradients(dep, t, (t > 0).float(), want_grad=False, fit_out=fits[k])
            if median:
                med, contrib = gsr.median_depth.render_median_depth(buf, c["height"], c["width"])
                mask = ((t > 0) & (contrib > 0).reshape(t.shape)).float()
                dm.append(float(gsr.loss.depth_loss_and_gradients(med.reshape(t.shape), t, mask, want_grad=False)[0].item()) / t.numel())
            if plane:
                pd = gsr.plane_depth.render_view_plane_depth(P, c, buf)[0]
                dp.append(float(gsr.loss.depth_loss_and_gradients(pd.reshape(t.shape), t, (t > 0).float(), want_grad=False)[0].item()) / t.numel())
            if plane_median:
                med, contrib = gsr.plane_depth.render_view_plane_median_depth(P, c, buf)[:2]
                mask = ((t > 0) & (contrib > 0).reshape(t.shape)).float()
                dpm.append(float(gsr.loss.depth_loss_and_gradients(med.reshape(t.shape), t, mask, want_grad=False)[0].item()) / t.numel())
            if clean_depth_targets is not None:
                t = clean_depth_targets[k]
                dc.append(float(gsr.loss.depth_loss_and_gradients(dep, t, (t > 0).float(), want_grad=False)[0].item()) / t.numel())
        if alpha_targets is not None:
            t = alpha_targets[k]
            al.append(float(gsr.loss.alpha_loss_and_gradients(buf["final_Ts"], t, want_grad=False)[0].item()) / t.numel())
    extra = {}
    if fits is not None:
        f = fits.cpu().numpy().astype(np.float64)
        extra = {"train_depth_corr_mean": float(f[:, 0].mean()), "train_depth_fit": [[float(s), float(b)] for s, b in f[:, 1:3]]}
        if dc:
            extra["train_depth_l1_clean_mean"] = float(np.mean(dc))
        if dm:
            extra["train_median_depth_l1_mean"] = float(np.mean(dm))
        if dp:
            extra["train_plane_depth_l1_mean"] = float(np.mean(dp))
        if dpm:
            extra["train_plane_median_depth_l1_mean"] = float(np.mean(dpm))
    return (float(np.mean(dl)) if dl else None), (float(np.mean(al)) if al else None), extra


def normal_scores(P, cams, normal_targets, normal_rots, bg, mode_kw, alpha_min):
    """{"train_normal_angle_deg_mean": the mean angle between the normals of the rendered depth (include/gsr_normals.h) and the targets
    over the pixels where both exist, averaged over the views that have such pixels; "train_normal_valid_share": the share of pixels
    with a valid depth normal, averaged over the views}."""
    angles, shares = [], []
    for c, t, R in zip(cams, normal_targets, normal_rots):
        _, dep, buf = gsr.render_view(P, c, bg, **mode_kw)
        n, valid = gsr.normals.normals_from_depth(dep.reshape(c["height"], c["width"]), buf["final_Ts"].reshape(c["height"], c["width"]), c, alpha_min)
        th = t.reshape(c["height"], c["width"], 3).double()
        if R is not None:
            th = th @ torch.as_tensor(np.asarray(R, np.float64).T, device=th.device)
        length = th.norm(dim=-1)
        both = (valid > 0) & (length > 0)
        shares.append(float(valid.mean().item()))
        if bool(both.any()):
            cos = ((n.double() * th).sum(-1)[both] / length[both]).clamp(-1.0, 1.0)
            angles.append(float(torch.rad2deg(torch.acos(cos)).mean().item()))
    return {"train_normal_angle_deg_mean": float(np.mean(angles)) if angles else None, "train_normal_valid_share": float(np.mean(shares))}


def distortion_score(P, cams, bg, mode_kw):
    """{"train_distortion_mean": the mean of the depth-distortion image (include/gsr_distortion.h) over pixels and views}"""
    means = [gsr.distortion.render_distortion(gsr.render_view(P, c, bg, **mode_kw)[2], c["height"], c["width"])[0].mean() for c in cams]
    return {"train_distortion_mean": float(torch.stack(means).double().mean().item())}


def normal_consistency_score(P, cams, bg, mode_kw, alpha_min):
    """{"train_normal_consistency_deg": the mean angle in degrees between N / |N|, N the blended image of the Gaussians' own normals
    (include/gsr_normal_render.h), and the normals of the rendered depth, over the counted pixels of all views (None: no such pixel)}"""
    total, count = 0.0, 0
    for c in cams:
        H, W = c["height"], c["width"]
        _, dep, buf = gsr.render_view(P, c, bg, **mode_kw)
        nimg = gsr.normal_render.render_normals(gsr.normal_render.gaussian_normals(P["scales"], P["rotations"], P["positions"], c), buf, H, W)
        n_d, valid = gsr.normals.normals_from_depth(dep.reshape(H, W), buf["final_Ts"].reshape(H, W), c, alpha_min)
        length = nimg.norm(dim=-1)
        counted = (valid > 0) & (length >= gsr._lib.NORMAL_RENDER_MIN_LENGTH)
        if bool(counted.any()):
            cos = ((n_d.double() * nimg.double()).sum(-1)[counted] / length.double()[counted]).clamp(-1.0, 1.0)
            total += float(torch.rad2deg(torch.acos(cos)).sum().item())
            count += int(counted.sum().item())
    return {"train_normal_consistency_deg": total / count if count else None}


def pose_errors(run):
    """--pose-noise-* / --optimize-poses: every view's error against the dataset poses (degrees, scene units) at the start and now"""
    V = run.views
    e0, e1 = ([gsr.pose.pose_error(c, t) for c, t in zip(cams, V.true_cams)] for cams in (V.start_cams, V.cams))
    return {"pose_error_start": {"rot_deg": [r for r, _ in e0], "trans": [t for _, t in e0]},
            "pose_error_final": {"rot_deg": [r for r, _ in e1], "trans": [t for _, t in e1]},
            "pose_rot_deg_mean_start": row_mean(e0, 0), "pose_trans_mean_start": row_mean(e0, 1),
            "pose_rot_deg_mean_final": row_mean(e1, 0), "pose_trans_mean_final": row_mean(e1, 1)}


def finish(run, wall):
    """The run record: parameters finite, loss curve, point count after every density-control call, timing, per-view scores, PNGs."""
    from PIL import Image
    args, V, model, bg, mode_kw, expo = run.args, run.views, run.model, run.bg, run.mode_kw, run.expo
    P, cams, targets = model.params, V.cams, V.targets
    finite = {k: bool(torch.isfinite(P[k]).all().item()) for k in gsr.optimizer.GROUPS}
    rows, images = score_views(P, cams, targets, bg, mode_kw, expo)
    summary = {"iterations": args.iterations, "wall_s": round(wall, 3), "iterations_per_s": round(args.iterations / wall, 1) if wall > 0 else None,
               "points_start": run.density_log[0]["points"], "points_final": model.num_points, "density_control_calls": len(run.density_log) - 1,
               "parameters_finite": finite, "train_views": rows, **row_means(rows, "train")}
    if args.capacity:
        summary["capacity_retries"] = len(run.capacity_log)
    if V.weights is not None:                                               # the same three scores under each view's weights
        wrows = [weighted_scores(img, t.reshape(img.shape), w) for img, t, w in zip(images, targets, V.weights)]
        summary.update({"train_views_weighted": wrows, **row_means(wrows, "train_weighted")})
    if V.clean_targets is not None:                                         # --occluders: against the targets before the rectangles
        crows, _ = score_views(P, cams, V.clean_targets, bg, mode_kw, expo)
        summary.update({"clean_views": crows, **row_means(crows, "clean")})
    if V.true_cams is not V.start_cams or args.optimize_poses:
        summary.update(pose_errors(run))
    if expo is not None:                                                    # --optimize-exposure: which rows went through a matrix, and the matrices
        summary["exposure_applied"] = {"train_views": True, "train_eval_scales": True, "holdout_views": False, "holdout_eval_scales": False}
        summary["exposure_final"] = expo.state_dict()["E"]
        summary["exposure_steps"] = list(expo.steps)
    d_l1, a_l1, d_extra = aux_scores(P, cams, V.depth_targets, V.alpha_targets, bg, mode_kw, V.clean_depth_targets, median=args.depth_render == "median",
                                      plane=args.depth_render == "plane", plane_median=args.depth_render == "plane-median")
    if args.depth_render != "expected":
        summary["depth_render"] = args.depth_render
    if d_l1 is not None:
        summary["train_depth_l1_mean"] = d_l1
    summary.update(d_extra)
    if a_l1 is not None:
        summary["train_alpha_l1_mean"] = a_l1
    if V.clean_normal_targets is not None:                                  # --lambda-normal / --normal-dir / the hidden scene's own
        summary.update(normal_scores(P, cams, V.clean_normal_targets, V.normal_rots, bg, mode_kw, args.normal_alpha_min))
    if args.lambda_dist > 0.0 or args.report_distortion:
        summary.update(distortion_score(P, cams, bg, mode_kw))
    if args.lambda_normal_consistency > 0.0 or args.report_normal_consistency:
        summary.update(normal_consistency_score(P, cams, bg, mode_kw, args.normal_alpha_min))
    if args.holdout and args.dataset:
        split, _, k = args.holdout.partition(":")
        hc, ht = load_nerf(args.dataset, int(k or 8), split)
        ht = [torch.as_tensor(t).to(run.dev) for t in ht]
        hrows, _ = score_views(P, hc, ht, bg, mode_kw)
        if V.eval_scales:
            summary["holdout_eval_scales"] = score_scales(P, hc, ht, bg, mode_kw, V.eval_scales)
        summary.update({"holdout": args.holdout, "holdout_views": hrows, **row_means(hrows, "holdout")})
    if V.eval_scales:
        summary["train_eval_scales"] = score_scales(P, cams, targets, bg, mode_kw, V.eval_scales, expo)
        for name in ("train_eval_scales", "holdout_eval_scales"):
            if name in summary:
                print(name + ": " + "; ".join(f"1/{k}: PSNR {v['psnr']:.2f} dB SSIM {v['ssim']:.4f}" for k, v in summary[name].items()), flush=True)
    print(f"trained {args.iterations} iterations in {wall:.2f} s ({summary['iterations_per_s']} it/s); {summary['points_start']} -> "
          f"{model.num_points} points; train L1 {summary['train_l1_mean']:.5f} PSNR {summary['train_psnr_mean']:.2f} dB"
          + (f"; holdout PSNR {summary['holdout_psnr_mean']:.2f} dB" if "holdout_psnr_mean" in summary else "")
          + f"; parameters finite: {all(finite.values())}", flush=True)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        curve = run.loss_hist[:args.iterations].cpu().numpy()
        scurve = run.ssim_hist[:args.iterations].cpu().numpy() if run.ssim_hist is not None else None
        with open(args.log, "w") as f:
            f.write(json.dumps({"record": "arguments", **{k: v for k, v in vars(args).items()}, **run.init_info}) + "\n")
            for kind, log in (("density_control", run.density_log), ("capacity_retry", run.capacity_log), ("filter_3d", run.filter_log)):
                for d in log:
                    f.write(json.dumps({"record": kind, **d}) + "\n")
            for i in range(0, len(curve), 100):               # every iteration's loss, 100 per line
                rec = {"record": "loss", "from_iteration": i, "l1": [round(float(x), 6) for x in curve[i:i + 100]]}
                if scurve is not None:                        # --lambda-dssim > 0: the mean SSIM of the same iterations
                    rec["ssim"] = [round(float(x), 6) for x in scurve[i:i + 100]]
                f.write(json.dumps(rec) + "\n")
            f.write(json.dumps({"record": "summary", **summary}) + "\n")
    if args.eval_dir:
        os.makedirs(args.eval_dir, exist_ok=True)
        to8 = lambda x: (x.clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).cpu().numpy()
        for k in range(min(args.eval_views, len(images))):
            r8, t8 = to8(images[k]), to8(targets[k].reshape(images[k].shape))
            Image.fromarray(r8).save(os.path.join(args.eval_dir, f"render_{k}.png"))
            Image.fromarray(t8).save(os.path.join(args.eval_dir, f"target_{k}.png"))
            Image.fromarray(np.concatenate([r8, t8], axis=1)).save(os.path.join(args.eval_dir, f"pair_{k}.png"))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1, help="ranks (one per GPU); > 1 without WORLD_SIZE launches them itself")
    ap.add_argument("--dataset", default=None)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--gaussians", type=int, default=5000)      # reference default (config.py:31)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--views-per-step", type=int, default=1)
    ap.add_argument("--view-streams", type=int, default=0, help="when a rank has several views per step (--views-per-step beyond the "
                    "number of GPUs), render up to this many at once on separate HIP streams (1 = one after the other; 0 = decide by "
                    "scene size each step: 3 from 2^17 Gaussians up -- +9 %% at 1 M Gaussians, profiles/r04_c_views_per_gpu.txt -- and 1 "
                    "below, where a step is host-bound and the extra stream hand-overs cost more than they hide: 872 against 750 "
                    "iterations/s at 6 000 Gaussians)")
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--densify-from", type=int, default=500)    # train.py:391-394 defaults
    ap.add_argument("--densify-until", type=int, default=15000)
    ap.add_argument("--densify-interval", type=int, default=100)
    ap.add_argument("--opacity-reset-interval", type=int, default=3000)
    ap.add_argument("--save-interval", type=int, default=500)   # config.py:32
    ap.add_argument("--init", default=None, choices=["reference", "random", "knn"], help="initial Gaussians: the reference's "
                    "init_gaussian_params (the default), a seeded random scene, or knn: the reference's positions with the scale of "
                    "each set from its three nearest neighbours (include/gsr_knn.h), the original 3DGS start from random points")
    ap.add_argument("--init-points", default=None, metavar="FILE.ply", help="start from the points of a binary little-endian PLY "
                    "(x y z, optional uchar red green blue): kNN scales, opacity 0.1, the colours in the SH DC term.  The point "
                    "count comes from the file (--gaussians is overridden); not with an explicit --init reference or --init random")
    ap.add_argument("--backend", default=None, help="collective backend (default: nccl = RCCL); gloo + --single-device rehearses N ranks on one GPU")
    ap.add_argument("--single-device", action="store_true")
    ap.add_argument("--dense-sh", action="store_true", help="materialise the 48-float SH gradient (backward's dense return, one "
                    "59-float all-reduce when N > 1) instead of forming it inside the Adam update from the view payloads")
    ap.add_argument("--output", default=None, help="directory for point_cloud/iteration_N/point_cloud.ply")
    ap.add_argument("--print-interval", type=int, default=10, help="iterations between loss lines (each one reads the loss back: a sync)")
    ap.add_argument("--log", default=None, help="JSONL run record: one line per density-control call, the per-iteration loss curve, "
                    "and a closing summary (wall time, iterations/s, per-view L1 / PSNR)")
    ap.add_argument("--eval-dir", default=None, help="after training, write render_<k>.png / target_<k>.png / pair_<k>.png for --eval-views")
    ap.add_argument("--eval-views", type=int, default=1, help="how many of the training views --eval-dir renders to PNG")
    ap.add_argument("--holdout", default=None, help="NeRF-synthetic split to score after training without training on it, e.g. "
                    "'test:8' = the first 8 frames of transforms_test.json (needs --dataset)")
    ap.add_argument("--capacity", action="store_true", help="capacity-mode forward (include/gsr_capacity.h): no host wait for the pair "
                    "count D.  The first iteration and any iteration after the point count changes render with the sized path to learn "
                    "D; the others with K = ceil(1.25 x the largest D seen).  The count is checked after backward() is enqueued, before "
                    "Adam; an overflowed view grows K and is run again with the sized path (a capacity_retry record in --log)")
    ap.add_argument("--capacity-initial", type=int, default=None, help="with --capacity: start with this K instead of a sized first iteration")
    ap.add_argument("--lambda-dssim", type=float, default=0.0, help="train on (1 - lambda) L1 + lambda (1 - SSIM) (include/gsr_loss.h; "
                    "standard 3DGS uses 0.2).  0 = L1 alone, the reference trainer's loss")
    ap.add_argument("--ssim-window", default="gaussian", choices=["gaussian", "reference"], help="SSIM window of the D-SSIM term: the "
                    "centred sigma = 1.5 Gaussian of standard 3DGS, or the reference's distance-indexed weights (gsr_ssim)")
    ap.add_argument("--lambda-depth", type=float, default=0.0, help="weight of the depth term: the masked inverse-depth L1 "
                    "(include/gsr_aux_grads.h), or what --depth-loss selects")
    ap.add_argument("--depth-loss", default="l1", choices=["l1", "pearson"], help="l1: the masked L1 against inverse depth in the scene's "
                    "own units.  pearson: 1 - the Pearson correlation of the rendered inverse depth with the target over the mask "
                    "(include/gsr_depth_corr.h), for relative targets: inverse depth known only up to an unknown scale a > 0 and shift b "
                    "per image (t -> a t + b), as monocular depth networks give it.  Needs --lambda-depth > 0; not divided by W H")
    ap.add_argument("--depth-render", default="expected", choices=["expected", "median", "plane", "plane-median"], help="the rendered inverse depth --lambda-depth's "
                    "L1 is taken on: the forward's expected inverse depth, or the median inverse depth (include/gsr_median_depth.h: the "
                    "Gaussian at which the transmittance falls through one half), masked to the pixels that have one; its gradient is a "
                    "stage of the backward; or the plane depth (include/gsr_plane_depth.h: every flat Gaussian contributes the depth at which the "
                    "pixel's ray meets its plane), which --lambda-normal-consistency then takes its depth normals from too; or the plane depth "
                    "under the median rule (include/gsr_plane_median.h: the plane of the one Gaussian the median chooses), masked like median, "
                    "its gradient added after the backward.  Needs --depth-loss l1")
    ap.add_argument("--depth-noise", type=float, default=0.0, metavar="S", help="make every depth target relative once, at load: "
                    "a_v t + b_v on its masked pixels, a_v = exp(U(-S, S)), b_v = U(0, S) * mean(t over the mask) per view; the summary "
                    "then also scores the depth against the clean targets (train_depth_l1_clean_mean)")
    ap.add_argument("--depth-seed", type=int, default=0, help="seed of the depth perturbation")
    ap.add_argument("--depth-dir", default=None, help="with --dataset: one float32 (H, W) inverse-depth .npy per frame, named after its "
                    "file_path (without --dataset the hidden scene's own inverse depth is the target)")
    ap.add_argument("--lambda-alpha", type=float, default=0.0, help="weight of the L1 of the alpha image 1 - final_T against the PNG "
                    "alpha (or the hidden scene's)")
    ap.add_argument("--lambda-normal", type=float, default=0.0, help="weight of the normal term: the cosine loss between the normals of "
                    "the rendered depth and a normal prior (include/gsr_normals.h), normalised by W H as the depth term; its two "
                    "gradient images are added to those of --lambda-depth and --lambda-alpha")
    ap.add_argument("--lambda-dist", type=float, default=0.0, metavar="W", help="weight of the depth-distortion term: W times the mean over "
                    "the pixels of sum_i sum_{j<i} w_i w_j (m_i - m_j)^2, m the inverse view depth (include/gsr_distortion.h); no target needed")
    ap.add_argument("--dist-from-iter", type=int, default=0, metavar="K", help="--lambda-dist acts from iteration K on")
    ap.add_argument("--report-distortion", action="store_true", help="the summary reports train_distortion_mean (the mean of the "
                    "distortion image over pixels and views at the end) also without --lambda-dist")
    ap.add_argument("--lambda-normal-consistency", type=float, default=0.0, metavar="W", help="weight of the depth-normal consistency term: W "
                    "times the mean over the pixels of 1 - n_d . N / |N|, N the blended image of the Gaussians' own normals (the direction of each "
                    "Gaussian's shortest axis), n_d the normals of the rendered depth (include/gsr_normal_render.h); no target needed")
    ap.add_argument("--normal-consistency-from-iter", type=int, default=0, metavar="K", help="--lambda-normal-consistency acts from iteration K on")
    ap.add_argument("--report-normal-consistency", action="store_true", help="the summary reports train_normal_consistency_deg (the mean angle "
                    "between N / |N| and n_d over counted pixels and views at the end) also without --lambda-normal-consistency")
    ap.add_argument("--normal-dir", default=None, help="with --dataset: one float32 (H, W, 3) normal .npy per frame, named after its "
                    "file_path (without --dataset the normals of the hidden scene's own depth are the targets)")
    ap.add_argument("--normal-space", default="camera", choices=["camera", "world"], help="the space of --normal-dir's vectors: camera "
                    "(x right, y down, z forward; normals face the camera, z < 0) or world (turned by each view's rotation)")
    ap.add_argument("--normal-noise", type=float, default=0.0, metavar="S", help="perturb every normal target once, at load: N(0, S^2) added to "
                    "each component of every non-zero target vector (a noisy prior); the summary scores against the clean targets")
    ap.add_argument("--normal-seed", type=int, default=0, help="seed of the normal perturbation")
    ap.add_argument("--normal-alpha-min", type=float, default=0.5, help="a pixel has a depth normal where its own and its four neighbours' "
                    "alpha is at least this")
    ap.add_argument("--mesh-out", default=None, metavar="FILE", help="after the last iteration, fuse depth and colour renders of the training "
                    "views into a TSDF volume and write the extracted triangle mesh (include/gsr_tsdf.h; what examples/extract_mesh.py does). "
                    "Off by default; training itself is unchanged")
    ap.add_argument("--mesh-depth", default="expected", choices=["expected", "median", "plane", "plane-median"], help="the depth --mesh-out fuses: "
                    "the expected inverse depth over the coverage, the median depth (include/gsr_median_depth.h), the plane depth "
                    "(include/gsr_plane_depth.h) or the plane depth under the median rule (include/gsr_plane_median.h)")
    ap.add_argument("--mesh-resolution", type=int, default=256, metavar="R", help="voxels per side of --mesh-out's volume")
    ap.add_argument("--mesh-min-weight", type=float, default=1.0, metavar="K", help="--mesh-out keeps cells whose corners all have weight K")
    ap.add_argument("--optimize-poses", action="store_true", help="refine each view's pose with Adam on the camera gradients "
                    "(include/gsr_camera_grads.h; one GPU; reads 35 floats back per view and iteration)")
    ap.add_argument("--pose-lr", type=float, default=1e-3, help="Adam learning rate of the pose corrections xi = (translation, "
                    "axis-angle rotation in radians), camera frame (pose.py)")
    ap.add_argument("--pose-noise-deg", type=float, default=0.0, help="perturb every dataset pose by this rotation (degrees, random axis)")
    ap.add_argument("--pose-noise-trans", type=float, default=0.0, help="... and this translation (scene units, random direction)")
    ap.add_argument("--pose-seed", type=int, default=0, help="seed of the pose perturbation")
    ap.add_argument("--densify-stat", default="reference", choices=["reference", "screen"], help="what density control tests: the "
                    "reference's 3D position gradient of the last view, or the screen-space gradient norm averaged over the views that "
                    "saw each Gaussian since the last call (include/gsr_densify_stats.h)")
    ap.add_argument("--absgrad", action="store_true", help="with --densify-stat screen: accumulate absolute per-pixel gradients "
                    "(backward(absgrad=True)); choose --densify-grad-threshold 2-4x the signed one")
    ap.add_argument("--densify-grad-threshold", type=float, default=0.0002, help="gradient threshold of clone / split (config.py:54)")
    ap.add_argument("--prune-screen-size", type=float, default=0.0, metavar="PX", help="with --densify-stat screen: prune Gaussians whose "
                    "largest screen radius exceeded PX pixels (0 = off; applies after the first opacity reset)")
    ap.add_argument("--prune-world-size", type=float, default=0.0, metavar="FRAC", help="with --densify-stat screen: prune Gaussians whose "
                    "largest scale exceeds FRAC of the scene extent (0 = off; applies after the first opacity reset)")
    ap.add_argument("--rasterize-mode", default="classic", choices=["classic", "antialiased"], help="antialiased: every Gaussian is drawn "
                    "with its opacity scaled by sqrt(det(Sigma2D) / det(Sigma2D + 0.3 I)), forward and backward (include/gsr_antialias.h); "
                    "training, evaluation and target renders all use the mode")
    ap.add_argument("--filter-3d", action="store_true", help="train under Mip-Splatting's 3D smoothing filter (include/gsr_filter3d.h): "
                    "every Gaussian is rendered with scales sqrt(s^2 + f^2) and its opacity scaled to keep its integral, f from the "
                    "sampling rate of all training cameras; recomputed before the first iteration, after every density-control call "
                    "that changes the point set, after an opacity reset, and every --filter-3d-interval iterations once density control "
                    "has ended.  Density control and pruning keep testing the raw parameters; checkpoints hold the fused ones")
    ap.add_argument("--filter-3d-variance", type=float, default=0.2, help="variance of the 3D filter in squared sampling intervals")
    ap.add_argument("--filter-3d-interval", type=int, default=100, help="iterations between recomputations after density control has ended")
    ap.add_argument("--eval-scales", default="", metavar="S,S,...", help="after training, also score every scored view (the training views, "
                    "and --holdout's) rendered at W/s x H/s with the same field of view against its target box-averaged by s x s; "
                    "PSNR and SSIM per scale go to the summary.  Every s must divide W and H")
    ap.add_argument("--optimize-exposure", action="store_true", help="learn an affine colour transform per training view (include/"
                    "gsr_exposure.h: 12 numbers, c' = c A + b), applied to the render before the loss, with Adam beside the Gaussians; no "
                    "host wait is added to the step.  Training views are scored through their matrix, --holdout views with the identity; "
                    "the matrices go to the summary and to exposure.json beside each PLY.  One GPU; not with --capacity")
    ap.add_argument("--exposure-lr-init", type=float, default=0.01, help="Adam learning rate of the exposure matrices at the first iteration")
    ap.add_argument("--exposure-lr-final", type=float, default=0.001, help="... and at the last (geometric decay, scheduler.decayed_lr)")
    ap.add_argument("--exposure-noise", type=float, default=0.0, metavar="S", help="replace every training target once, at load, by "
                    "clamp(t A_v + b_v, 0, 1): A_v = diag(exp(u_v + w_v)), u_v ~ N(0, S^2) per channel, w_v ~ N(0, S^2) shared, "
                    "b_v ~ N(0, (S/4)^2) per channel (exposure.random_exposures)")
    ap.add_argument("--exposure-seed", type=int, default=0, help="seed of the exposure perturbation")
    ap.add_argument("--mask-dir", default=None, help="with --dataset: per-pixel weights of the colour loss (include/gsr_weighted_loss.h), "
                    "<DIR>/<basename of file_path>.png per training view, first channel / 255 (0 = the pixel does not count); the shape "
                    "must be the image's")
    ap.add_argument("--mask-dilate", type=int, default=5, metavar="R", help="grow the ignored region of every mask by R pixels first "
                    "(the minimum over each (2R+1)^2 neighbourhood).  5 is the SSIM window's radius: what the grown mask covers is then "
                    "invisible to the D-SSIM term too")
    ap.add_argument("--occluders", type=int, default=0, metavar="K", help="paste K opaque rectangles of a random saturated colour into "
                    "every training target once, at load, elsewhere in every view; the summary also scores against the clean targets")
    ap.add_argument("--occluder-seed", type=int, default=0, help="seed of the rectangles")
    ap.add_argument("--occluder-size", type=float, default=0.25, metavar="F", help="largest side of a rectangle, as a fraction of the image's")
    ap.add_argument("--mask-occluders", action="store_true", help="train with the masks of exactly those rectangles (dilated by --mask-dilate)")
    return ap.parse_args(argv)


def check_args(args):
    """Every refusal that needs no data, before anything touches the GPU, in the order that decides which message a doubly wrong
    command line gets.  --init-points is read here, where its refusals stand: returns its (points, colours) or None, and settles
    args.init and args.gaussians."""
    if args.init_points and args.init in ("reference", "random"):
        raise SystemExit(f"--init-points starts from the file's points: it cannot be combined with --init {args.init}")
    init_cloud = None
    if args.init_points:
        try:
            init_cloud = gsr.point_cloud.load_points(args.init_points)
        except (ValueError, OSError) as e:
            raise SystemExit(f"--init-points: {e}") from None
        if len(init_cloud[0]) < 1:
            raise SystemExit("--init-points: the file holds no points")
        print(f"--init-points: {len(init_cloud[0])} points from {args.init_points} (--gaussians {args.gaussians} is overridden)", flush=True)
        args.gaussians, args.init = len(init_cloud[0]), "points"
    args.init = args.init or "reference"
    finite = lambda *xs: bool(np.isfinite(sum(xs)))
    refuse([
        (args.mask_dilate < 0 or args.occluders < 0 or not 0.0 < args.occluder_size <= 1.0,
         "--mask-dilate and --occluders must be >= 0, --occluder-size in (0, 1]"),
        (args.mask_dir and not args.dataset, "--mask-dir needs --dataset (the masks are named after its frames)"),
        (args.mask_occluders and args.occluders == 0, "--mask-occluders needs --occluders K"),
        (not (args.exposure_lr_init > 0.0 and args.exposure_lr_final > 0.0 and finite(args.exposure_lr_init, args.exposure_lr_final)),
         "--exposure-lr-init and --exposure-lr-final must be positive and finite"),
        (not (args.exposure_noise >= 0.0 and finite(args.exposure_noise)), "--exposure-noise must be >= 0 and finite"),
        (args.optimize_exposure and args.capacity,
         "--optimize-exposure does not combine with --capacity (an overflowed frame's exposure step would have to be undone): drop one"),
        (not (args.filter_3d_variance > 0.0 and finite(args.filter_3d_variance)) or args.filter_3d_interval < 1,
         "--filter-3d-variance must be positive and finite, --filter-3d-interval >= 1")])
    if not args.dataset:
        parse_eval_scales(args.eval_scales, args.size, args.size)          # (a dataset's size is known once it is loaded)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    refuse([
        (not args.densify_grad_threshold >= 0.0 or not args.prune_screen_size >= 0.0 or not args.prune_world_size >= 0.0,
         "--densify-grad-threshold, --prune-screen-size and --prune-world-size must be >= 0"),
        (args.densify_stat != "screen" and (args.absgrad or args.prune_screen_size > 0.0 or args.prune_world_size > 0.0),
         "--absgrad, --prune-screen-size and --prune-world-size need --densify-stat screen"),
        (not args.pose_lr >= 0.0 or not args.pose_noise_deg >= 0.0 or not args.pose_noise_trans >= 0.0,
         "--pose-lr, --pose-noise-deg and --pose-noise-trans must be >= 0"),
        (not args.lambda_depth >= 0.0 or not args.lambda_alpha >= 0.0, "--lambda-depth and --lambda-alpha must be >= 0"),
        (args.mesh_out and not 2 <= args.mesh_resolution <= 2048, "--mesh-resolution must be in 2 .. 2048"),
        (args.mesh_out and not args.mesh_min_weight > 0.0, "--mesh-min-weight must be positive"),
        (not (args.lambda_normal >= 0.0 and finite(args.lambda_normal)), "--lambda-normal must be >= 0 and finite"),
        (not (args.normal_noise >= 0.0 and finite(args.normal_noise)), "--normal-noise must be >= 0 and finite"),
        (not (args.lambda_dist >= 0.0 and finite(args.lambda_dist)), "--lambda-dist must be >= 0 and finite"),
        (not args.dist_from_iter >= 0, "--dist-from-iter must be >= 0"),
        (not (args.lambda_normal_consistency >= 0.0 and finite(args.lambda_normal_consistency)), "--lambda-normal-consistency must be >= 0 and finite"),
        (not args.normal_consistency_from_iter >= 0, "--normal-consistency-from-iter must be >= 0"),
        (not finite(args.normal_alpha_min), "--normal-alpha-min must be finite"),
        (args.normal_dir and not args.dataset, "--normal-dir needs --dataset (the targets are named after its frames)"),
        (args.lambda_normal > 0.0 and args.dataset and not args.normal_dir, "--lambda-normal with --dataset needs --normal-dir (normal targets)"),
        (args.depth_loss == "pearson" and not args.lambda_depth > 0.0, "--depth-loss pearson needs --lambda-depth > 0 (its weight)"),
        (args.depth_render == "median" and args.depth_loss != "l1", "--depth-render median needs --depth-loss l1"),
        (args.depth_render == "plane" and args.depth_loss != "l1", "--depth-render plane needs --depth-loss l1"),
        (args.depth_render == "plane-median" and args.depth_loss != "l1", "--depth-render plane-median needs --depth-loss l1"),
        (not (args.depth_noise >= 0.0 and finite(args.depth_noise)), "--depth-noise must be >= 0 and finite"),
        (args.depth_noise > 0.0 and args.dataset and not args.depth_dir,
         "--depth-noise with --dataset needs --depth-dir (there is no depth target to perturb)"),
        (args.lambda_depth > 0.0 and args.dataset and not args.depth_dir, "--lambda-depth with --dataset needs --depth-dir (inverse-depth targets)"),
        (not 0.0 <= args.lambda_dssim <= 1.0, f"--lambda-dssim must be in [0, 1], not {args.lambda_dssim}"),
        (args.capacity_initial is not None and not (args.capacity and 0 <= args.capacity_initial <= (1 << 30)),
         "--capacity-initial needs --capacity and a value in [0, 2^30]"),
        *(((args.gpus > 1 or world > 1) and getattr(args, flag), ONE_GPU_ONLY[flag]) for flag in ("optimize_poses", "optimize_exposure")),
        (args.gpus > 1 and world != args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"),
        (not 1 <= args.views_per_step <= args.views,
         f"--views-per-step {args.views_per_step} must be in 1..--views ({args.views}): a step draws its views without replacement")])
    return init_cloud


def open_device(args):
    """(dev, rank, world): this rank's GPU, and the process group when there are several ranks"""
    local = 0 if args.single_device else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    rank, world = 0, int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        rank, world = gsr.dist.init_from_env(backend=args.backend, device=dev)
    return dev, rank, world


def load_views(args, dev):
    """Everything the run holds per view, as one record: the cameras (`cams`: the current ones, a list --optimize-poses writes;
    `start_cams`: after --pose-noise-*; `true_cams`: the dataset's), the colour, alpha, depth and normal targets with their clean
    copies (None: that perturbation is off), `depth_masks`, `normal_rots`, `weights` (loss.PixelWeights or None) with their totals
    `w_total`, and `eval_scales`.  Targets: the dataset's, or renders of a hidden seeded scene.  The load-time perturbations follow
    in a fixed order, each on its own seeded stream."""
    bg, mode_kw = np.zeros(3, np.float32), mode_keywords(args)
    depth_targets = alpha_targets = normal_targets = None
    if args.dataset:
        cams, targets, alpha_targets, *dt = load_nerf(args.dataset, args.views, alpha=True, depth_dir=args.depth_dir)
        targets = [torch.as_tensor(t).to(dev) for t in targets]
        alpha_targets = [torch.as_tensor(t).to(dev) for t in alpha_targets]
        depth_targets = [torch.as_tensor(t).to(dev) for t in dt[0]] if dt else None
        if args.normal_dir:
            try:
                normal_targets = [torch.as_tensor(t).to(dev) for t in
                                  load_normals(args.dataset, args.normal_dir, args.views, [(c["height"], c["width"]) for c in cams])]
            except (ValueError, OSError) as e:
                raise SystemExit(f"--normal-dir: {e}") from None
    else:
        cams = [gsr.cameras.nerf_camera(gsr.scenes.orbit_pose(k, args.views), args.size, args.size, gsr.scenes.LEGO_CAMERA_ANGLE_X)
                for k in range(args.views)]
        hidden = gsr.scenes.synthetic_scene(args.gaussians, 0.05, 0.5, seed=7)
        hidden = {"positions": hidden["means"], "scales": hidden["scales"], "rotations": hidden["rotations"], "opacities": hidden["opacities"],
                  "shs": hidden["shs"]}
        targets, depth_targets, alpha_targets, normal_targets = [], [], [], []
        for c in cams:
            img, dep, hb = gsr.render_view(hidden, c, bg, **mode_kw)
            targets.append(img)
            depth_targets.append(dep.reshape(c["height"], c["width"]).clone())
            alpha_targets.append((1.0 - hb["final_Ts"].reshape(c["height"], c["width"])).contiguous())
            normal_targets.append(gsr.normals.normals_from_depth(dep.reshape(c["height"], c["width"]), hb["final_Ts"].reshape(c["height"], c["width"]),
                                                                 c, args.normal_alpha_min)[0])     # camera space; zero where it has none
    eval_scales = parse_eval_scales(args.eval_scales, cams[0]["width"], cams[0]["height"])
    if args.exposure_noise > 0.0:                                            # every target as a camera with that exposure error stored it
        noise = gsr.exposure.random_exposures(len(targets), args.exposure_noise, args.exposure_seed)
        targets = [gsr.exposure.perturbed_target(t.reshape(c["height"], c["width"], 3), e) for t, c, e in zip(targets, cams, noise)]
    masks = None                                                            # per view: the (H, W) weights as given, on the host
    if args.mask_dir:
        try:
            masks = load_masks(args.dataset, args.mask_dir, args.views, [(c["height"], c["width"]) for c in cams])
        except (ValueError, OSError) as e:
            raise SystemExit(f"--mask-dir: {e}") from None
    clean_targets = None
    if args.occluders > 0:                                                  # every target as a capture with things in the way stored it
        clean_targets, pasted = targets, []
        if args.mask_occluders and masks is None:
            masks = [np.ones((c["height"], c["width"]), np.float32) for c in cams]
        for v, (t, c) in enumerate(zip(targets, cams)):
            rects = occluder_rects(c["height"], c["width"], args.occluders, args.occluder_size, args.occluder_seed, v)
            img, hole = paste_occluders(t.reshape(c["height"], c["width"], 3).cpu().numpy(), rects)
            pasted.append(torch.as_tensor(img).to(dev))
            if args.mask_occluders:
                masks[v] = masks[v] * hole
        targets = pasted
    weights = w_total = None                                                # per view: loss.PixelWeights (the grown mask and its total M_v)
    if masks is not None:
        weights = [gsr.loss.PixelWeights(torch.as_tensor(m).to(dev), dilate=args.mask_dilate) for m in masks]
        w_total = [float(p.total.item()) for p in weights]
        if min(w_total) <= 0.0:
            raise SystemExit(f"the mask of view {int(np.argmin(w_total))} leaves no pixel with weight (after --mask-dilate {args.mask_dilate})")
    # --pose-noise-*: the poses the trainer starts from; the dataset's stay in true_cams for the pose error (the targets are the
    # dataset's images, or renders of the hidden scene from the dataset poses)
    true_cams = cams
    if args.pose_noise_deg > 0.0 or args.pose_noise_trans > 0.0:
        prng = np.random.default_rng(args.pose_seed)
        cams = [gsr.pose.apply_pose_delta(c, gsr.pose.random_pose_delta(prng, args.pose_noise_deg, args.pose_noise_trans)) for c in cams]
    depth_masks = [(t > 0).float() for t in depth_targets] if depth_targets is not None else None   # (from the clean targets)
    clean_depth_targets = None
    if args.depth_noise > 0.0:                                              # every depth target as a relative depth source stored it
        clean_depth_targets, depth_targets = depth_targets, perturb_depth_targets(depth_targets, args.depth_noise, args.depth_seed)
    # the rotation that takes each view's normal targets to camera space (None: they are there already)
    normal_rots = [c["R"] if args.dataset and args.normal_space == "world" else None for c in cams] if normal_targets is not None else None
    clean_normal_targets = normal_targets
    if args.normal_noise > 0.0 and normal_targets is not None:              # every normal target as a noisy prior stored it
        gen = torch.Generator(device="cpu").manual_seed(args.normal_seed)
        normal_targets = [torch.where((t != 0).any(-1, keepdim=True), t + args.normal_noise * torch.randn(t.shape, generator=gen).to(dev), t).contiguous()
                          for t in normal_targets]
    return SimpleNamespace(
        cams=list(cams), start_cams=cams, true_cams=true_cams, targets=targets, clean_targets=clean_targets, alpha_targets=alpha_targets,
        depth_targets=depth_targets, clean_depth_targets=clean_depth_targets, depth_masks=depth_masks, normal_targets=normal_targets,
        clean_normal_targets=clean_normal_targets, normal_rots=normal_rots, weights=weights, w_total=w_total, eval_scales=eval_scales,
        sum_scale=float(cams[0]["height"] * cams[0]["width"] * 3))          # an unweighted L1 sum -> mean (all views of a dataset share one size)


def init_params(args, dev, cloud):
    """(P, init_info): the Gaussians the run starts from (--init, or --init-points' cloud) and what the --log header says of them"""
    n = args.gaussians
    if args.init == "reference":
        # the reference trainer's start (train.py:37-92, 193-214): randf-hashed positions in (-1.3, 1.3)^3, scale 0.1, opacity 0.1
        P = gsr.densify.init_gaussian_params(n, 0.1, dev)
    elif args.init == "knn":
        # the same positions, every scale from the point's three nearest neighbours: the original's start from random points
        P = gsr.densify.init_gaussian_params(n, 0.1, dev)
        P["scales"].copy_(gsr.knn.init_scales(P["positions"]))
    elif args.init == "points":
        P = gsr.point_cloud.gaussians_from_points(cloud[0], cloud[1], device=dev)
    else:
        init = gsr.scenes.synthetic_scene(n, 0.05, 0.5, seed=8)             # same on every rank (replicated parameters)
        t = lambda a, shape: torch.as_tensor(np.ascontiguousarray(a, np.float32)).reshape(shape).to(dev)
        P = {"positions": t(init["means"], (n, 3)), "scales": t(init["scales"], (n, 3)), "rotations": t(init["rotations"], (n, 4)),
             "opacities": t(init["opacities"], (n,)), "shs": t(init["shs"], (n * 16, 3))}
    init_info = {"init": args.init}
    if args.init in ("knn", "points"):
        s0 = P["scales"][:, 0]
        init_info.update({"init_scale_min": float(s0.min().item()), "init_scale_median": float(s0.median().item()),
                          "init_scale_max": float(s0.max().item())})
        print(f"--init {args.init}: {n} Gaussians, initial scale min {init_info['init_scale_min']:.4g} median "
              f"{init_info['init_scale_median']:.4g} max {init_info['init_scale_max']:.4g}", flush=True)
    return P, init_info


def new_run(args, dev, rank, world, views, P, init_info):
    """The run record: everything a step reads or writes beside the library's own state, made once."""
    model = gsr.densify.GaussianModel(
        P, scene_extent=gsr.densify.calculate_scene_extent([c["camera_center"] for c in views.cams]),
        config={"densify_from_iter": args.densify_from, "densify_until_iter": args.densify_until, "densification_interval": args.densify_interval,
                "opacity_reset_interval": args.opacity_reset_interval, "max_allowed_prune_ratio": 1.0, "background_color": [0.0, 0.0, 0.0],
                "densify_statistic": args.densify_stat, "densify_grad_threshold": args.densify_grad_threshold,
                "prune_screen_size": args.prune_screen_size, "prune_world_size": args.prune_world_size})
    n_views, dssim = len(views.cams), args.lambda_dssim > 0.0
    per_rank_views = -(-args.views_per_step // world)
    return SimpleNamespace(
        args=args, dev=dev, rank=rank, world=world, views=views, model=model, init_info=init_info, bg=np.zeros(3, np.float32),
        mode_kw=mode_keywords(args),
        # what the flags select, settled once.  The SH gradient is never materialised: backward() returns the 3-float view payload it
        # is an outer product of, the ranks exchange that (11 + 3 floats per Gaussian instead of 59, dist.py) and the Adam kernel forms
        # basis x payload inside the SH update (optimizer.adam_update(sh_views=...)) -- also with one rank.  --dense-sh keeps the
        # 48-float path.
        factored=not args.dense_sh, dssim=dssim, screen_stats=args.densify_stat == "screen", abs_kw={"absgrad": True} if args.absgrad else {},
        aux=args.lambda_depth > 0.0 or args.lambda_alpha > 0.0 or args.lambda_normal > 0.0 or args.lambda_normal_consistency > 0.0,
        sched={k: gsr.scheduler.LRScheduler(lr) for k, lr in gsr.optimizer.DEFAULT_LR.items()},
        rng=np.random.default_rng(0),                                       # same stream on every rank -> same view batch
        per_rank_views=per_rank_views, streams_few=gsr.dist.ViewStreams(1, dev),
        streams_many=gsr.dist.ViewStreams(min(per_rank_views, args.view_streams or 3), dev),
        expo=gsr.exposure.ExposureModel(n_views, dev) if args.optimize_exposure else None,
        # --optimize-poses: each view's correction xi and its Adam state
        pose=SimpleNamespace(xi=[np.zeros(6) for _ in range(n_views)], m=[np.zeros(6) for _ in range(n_views)],
                             v=[np.zeros(6) for _ in range(n_views)], t=[0] * n_views),
        # --capacity: K (None = render sized), the point count K was last confirmed for, the largest D seen, and each view's last D (its
        # shape hint: the backward's block shape then follows the view's own count, as on the sized path)
        cap={"K": args.capacity_initial, "n": model.num_points if args.capacity_initial is not None else None, "max_D": 0, "D_of": {}},
        density_log=[{"iteration": -1, "points": model.num_points}], capacity_log=[], filter_log=[],
        loss_hist=torch.zeros(max(1, args.iterations), device=dev),         # the loss curve stays on the device until the end
        ssim_hist=torch.zeros(max(1, args.iterations), device=dev) if dssim else None,   # --lambda-dssim: the SSIM curve beside it
        ssim_of={},                                                         # (several views per rank: each view's mean SSIM)
        view_of=[])                                                         # (one view per rank and step: the view of every iteration)


def mean_divisor(run, v, host=True):
    """What divides an L1 sum over view v to give the view's mean; an SSIM sum's is a third of it.  Under per-pixel weights 3 M_v, M_v
    the view's weight total -- host=False: from the device scalar, no wait; v a list of views: the device vector of theirs -- else
    the 3 W H that all views share.  Where it is applied follows the step's layout: with one view per rank and step the loss
    kernel writes the SUMS into the curves' slots, which are divided when they are printed and once at the end (rescale_curves);
    with several, every view's sums are divided in the step and the slots hold means."""
    V = run.views
    if V.weights is None:
        return V.sum_scale
    if isinstance(v, list):
        return 3.0 * torch.tensor(V.w_total, device=run.dev)[torch.tensor(v, device=run.dev)]
    return 3.0 * (V.w_total[v] if host else V.weights[v].total)


def pose_step(run, v, grad):
    """One Adam step (beta 0.9 / 0.999, eps 1e-15) on view v's xi; its camera dict is rebuilt for the next render."""
    p, V = run.pose, run.views
    p.t[v] += 1
    p.m[v] = 0.9 * p.m[v] + 0.1 * grad
    p.v[v] = 0.999 * p.v[v] + 0.001 * grad * grad
    mh, vh = p.m[v] / (1.0 - 0.9 ** p.t[v]), p.v[v] / (1.0 - 0.999 ** p.t[v])
    p.xi[v] = p.xi[v] - run.args.pose_lr * mh / (np.sqrt(vh) + 1e-15)
    V.cams[v] = gsr.pose.apply_pose_delta(V.start_cams[v], p.xi[v])


def recompute_filter(run, it, why):
    """--filter-3d: the filter of the current point set from ALL training cameras at their current poses (every rank computes
    the same bits: no collective).  One record per call; its statistics are the one read-back."""
    model = run.model
    f = gsr.filter3d.compute_filter_3d(model.params["positions"], run.views.cams, run.args.filter_3d_variance)
    assert f.shape[0] == model.num_points == model.params["scales"].shape[0], (f.shape, model.num_points)
    run.mode_kw["filter_3d"] = f
    q = torch.stack((f.min(), f.median(), f.max())).tolist() if f.numel() else [0.0, 0.0, 0.0]
    run.filter_log.append({"iteration": it, "why": why, "points": model.num_points, "min": q[0], "median": q[1], "max": q[2]})


def train_view(run, it, v, alone, capacity=None):
    """One view of a step: render, the loss terms and their pixel gradients, backward.  Returns (loss, the gradient arena, the SH
    view payload, frame, dL/dxi).  `alone`: v is its rank's only view of the step -- the loss kernel then writes the sums into the
    curves' slots and `loss` is the L1 sum; otherwise it is the view's mean.  frame: None, and under --capacity (buffers, backward's
    dict): the frame's D, and for a capacity-mode frame (`capacity` = K) the screen statistics that capacity_views() adds only once
    the overflow check has passed.  dL/dxi: None, and under --optimize-poses this frame's pose gradient -- the caller takes the pose
    step (pose_step), once per view and iteration and only from a frame it trusts."""
    args, V, P, bg, mode_kw = run.args, run.views, run.model.params, run.bg, run.mode_kw
    c = V.cams[v]
    if capacity is None:
        img, dep, buf = gsr.render_view(P, c, bg, **mode_kw)
        run.init_info.setdefault("first_iteration_pairs", int(buf["point_list"].shape[0]))   # D of the run's first frame (sized: the host has it)
    else:
        img, dep, buf = gsr.render_view(P, c, bg, **mode_kw, capacity=capacity, capacity_hint=run.cap["D_of"].get(v, run.cap["max_D"]))
    raw, expo = img, run.expo
    if expo is not None:                                                # the loss (and its curve) sees the corrected render
        raw = img.reshape(c["height"], c["width"], 3)
        img = gsr.exposure.apply_exposure(raw, expo.matrix(v))
    w_v = V.weights[v] if V.weights is not None else None               # the colour loss under this view's weights (None: the plain call)
    mean_of = mean_divisor(run, v, host=False)
    loss_out = run.loss_hist[it:it + 1] if alone else None              # (alone: the L1 sum goes straight into this iteration's slot)
    if run.dssim:                                                       # ... and the SSIM sum into the SSIM curve's
        loss_sum, ssim_sum, dpix = gsr.loss.l1_dssim_loss_and_gradients(img, V.targets[v], args.lambda_dssim, args.ssim_window, loss_out=loss_out,
                                                                        ssim_out=run.ssim_hist[it:it + 1] if alone else None, weights=w_v)
        run.ssim_of[v] = ssim_sum / (mean_of / 3.0)                     # (a re-run of an overflowed view replaces its entry)
    else:
        loss_sum, dpix = gsr.loss.l1_loss_and_gradients(img, V.targets[v], loss_out=loss_out, weights=w_v)
    kw, plane_median = {}, None
    if args.lambda_depth > 0.0 and args.depth_loss == "pearson":        # lambda_d (1 - rho): blind to the target's scale and shift
        kw["dL_ddepth_image"] = gsr.loss.depth_corr_loss_and_gradients(dep, V.depth_targets[v], V.depth_masks[v], args.lambda_depth)[1]
    elif args.lambda_depth > 0.0 and args.depth_render == "median":     # the same L1 on the median inverse depth, where a pixel has one
        med, contrib = gsr.median_depth.render_median_depth(buf, c["height"], c["width"])
        t = V.depth_targets[v]
        mask = V.depth_masks[v] * (contrib > 0).reshape(t.shape)         # the target's mask and "this pixel has a median"
        kw["dL_dmedian_depth"] = gsr.loss.depth_loss_and_gradients(med.reshape(t.shape), t, mask, args.lambda_depth)[1]
        kw["median_contributor"] = contrib
    elif args.lambda_depth > 0.0 and args.depth_render == "plane-median":   # the same L1 on the plane depth under the median rule, masked as above
        pm_med, pm_contrib, pm_s, pm_n = gsr.plane_depth.render_view_plane_median_depth(P, c, buf)
        t = V.depth_targets[v]
        mask = V.depth_masks[v] * (pm_contrib > 0).reshape(t.shape)
        plane_median = (gsr.loss.depth_loss_and_gradients(pm_med.reshape(t.shape), t, mask, args.lambda_depth)[1], pm_contrib, pm_s, pm_n)
    elif args.lambda_depth > 0.0 and args.depth_render == "plane":      # the same L1 on the plane-depth image; its gradient is a stage of the backward
        plane_img, plane_s, plane_n = gsr.plane_depth.render_view_plane_depth(P, c, buf)
        g_plane = gsr.loss.depth_loss_and_gradients(plane_img.reshape(V.depth_targets[v].shape), V.depth_targets[v], V.depth_masks[v], args.lambda_depth)[1]
        kw.update(dL_dplane_depth=g_plane.reshape(c["height"], c["width"]), plane_slopes=plane_s, plane_depth_image=plane_img, gaussian_normals=plane_n)
    elif args.lambda_depth > 0.0:                                       # (the curve keeps the colour loss: the terms are in the summary)
        kw["dL_ddepth_image"] = gsr.loss.depth_loss_and_gradients(dep, V.depth_targets[v], V.depth_masks[v], args.lambda_depth)[1]
    if args.lambda_alpha > 0.0:
        kw["dL_dalpha_image"] = gsr.loss.alpha_loss_and_gradients(buf["final_Ts"], V.alpha_targets[v], None, args.lambda_alpha)[1]
    if args.lambda_normal > 0.0:                                        # its two images are ADDED to the depth and alpha terms'
        _, gD, gA = gsr.loss.normal_loss_and_gradients(dep.reshape(c["height"], c["width"]), buf["final_Ts"].reshape(c["height"], c["width"]),
                                                       V.normal_targets[v], c, None, args.lambda_normal, V.normal_rots[v], args.normal_alpha_min)
        kw["dL_ddepth_image"] = gD if "dL_ddepth_image" not in kw else kw["dL_ddepth_image"].reshape(gD.shape) + gD
        kw["dL_dalpha_image"] = gA if "dL_dalpha_image" not in kw else kw["dL_dalpha_image"].reshape(gA.shape) + gA
    # (under --capacity this frame's overflow check comes later, in capacity_views(): both distortion kernels bound every walk by
    # the capacity, so an overflowed frame gives wrong numbers, never a fault, and capacity_views() runs that view again, sized)
    if args.lambda_dist > 0.0 and it >= args.dist_from_iter:            # no image carries this gradient: a stage of the backward
        dist_image, moments = gsr.distortion.render_distortion(buf, c["height"], c["width"])
        kw["dL_ddistortion"] = gsr.loss.distortion_loss_and_gradients(dist_image, None, args.lambda_dist)[1]
        kw["distortion_moments"] = moments
    if args.lambda_normal_consistency > 0.0 and it >= args.normal_consistency_from_iter:
        # the Gaussians' own normals against the normals of the rendered depth, the gradient on both sides: the depth side's two
        # images are ADDED to the terms' above, the normal image's gradient is a stage of the backward (like the distortion's)
        H, W = c["height"], c["width"]
        if args.depth_render == "plane" and "plane_depth_image" not in kw:     # (no --lambda-depth: the plane depth serves this term alone)
            plane_img, plane_s, plane_n = gsr.plane_depth.render_view_plane_depth(P, c, buf)
            kw.update(dL_dplane_depth=torch.zeros_like(plane_img), plane_slopes=plane_s, plane_depth_image=plane_img, gaussian_normals=plane_n)
        gn = kw["gaussian_normals"] if "gaussian_normals" in kw else gsr.normal_render.gaussian_normals(P["scales"], P["rotations"], P["positions"], c)
        nimg = gsr.normal_render.render_normals(gn, buf, H, W)
        on_plane = "plane_depth_image" in kw                            # --depth-render plane: the depth normals come from the plane depth
        _, gN, gD, gA = gsr.loss.normal_consistency_loss_and_gradients(nimg, (kw["plane_depth_image"] if on_plane else dep).reshape(H, W),
                                                                       buf["final_Ts"].reshape(H, W), c, None,
                                                                       args.lambda_normal_consistency, args.normal_alpha_min)
        if on_plane:                                                    # ... and their depth-side gradient goes back to it
            kw["dL_dplane_depth"] = kw["dL_dplane_depth"] + gD.reshape(H, W)
        else:
            kw["dL_ddepth_image"] = gD if "dL_ddepth_image" not in kw else kw["dL_ddepth_image"].reshape(gD.shape) + gD
        kw["dL_dalpha_image"] = gA if "dL_dalpha_image" not in kw else kw["dL_dalpha_image"].reshape(gA.shape) + gA
        kw.update(dL_dnormal_image=gN, gaussian_normals=gn, normal_image=nimg)
    if expo is not None:                                                # dL/d(corrected) -> dL/d(render) in place, and this view's dL/dE
        dpix, dE = gsr.exposure.exposure_backward(raw, expo.matrix(v), dpix, out=dpix)
    if run.aux:                                                         # the forward's depths: records re-packed with 1/depth
        kw["geom_buffer"] = {"depths": buf["depths"]}
    g = gsr.backward_view(P, c, bg, buf, dpix, sh_gradient="factored" if run.factored else "dense", camera_grad=args.optimize_poses,
                          **kw, **run.abs_kw, **mode_kw)
    if plane_median is not None:                                        # no stage of the backward: three calls ADD into g's means and rotations
        g_pm, pm_contrib, pm_s, pm_n = plane_median
        gsr.plane_depth.plane_median_gradients(P, c, buf, g_pm.reshape(c["height"], c["width"]).contiguous(), pm_contrib, pm_s, pm_n, grads=g)
    if run.screen_stats and capacity is None:                           # this view's statistics, on this view's stream
        run.model.stats.update(buf["radii"], g, use_abs=args.absgrad)
    if expo is not None:                                                # one single-wave launch; no read-back
        expo.step(v, dE, gsr.scheduler.decayed_lr(args.exposure_lr_init, args.exposure_lr_final, it, args.iterations))
    dxi = None
    if args.optimize_poses:                                             # 35 floats back: the wait this flag accepts
        gv, gp, gc = torch.cat([g["dL_dviewmatrix"].view(-1), g["dL_dprojmatrix"].view(-1), g["dL_dcampos"]]).cpu().double().split([16, 16, 3])
        dxi = gsr.pose.pose_gradient(V.start_cams[v], run.pose.xi[v], gv.view(4, 4), gp.view(4, 4), gc)
    return (loss_sum if alone else loss_sum / mean_of), g["_arena"], g["_view_payload"], ((buf, g) if args.capacity else None), dxi


def capacity_views(run, it, mine, n):
    """--capacity: every view enqueued without a wait for D; then, with the backward enqueued and before Adam, each view's count
    is read (the GPU is long past the scan) and an overflowed view is run again with the sized path."""
    cap, alone = run.cap, len(mine) == 1
    sized = cap["K"] is None or cap["n"] != n
    out = []
    for v in mine:
        l_v, a_v, p_v, (buf, g), dxi = train_view(run, it, v, alone, None if sized else cap["K"])
        # (sized -- the first iteration, or the point count changed: the host has D, what K is learnt from)
        D, overflowed = (int(buf["point_list"].shape[0]), False) if sized else gsr.forward.rendered_count(buf)
        cap["D_of"][v] = D
        cap["max_D"] = max(cap["max_D"], D)
        if overflowed:                                                  # nothing computed from that frame is trusted
            run.capacity_log.append({"iteration": it, "view": v, "capacity": cap["K"], "D": D})
            l_v, a_v, p_v, _, dxi = train_view(run, it, v, alone)
        elif run.screen_stats and not sized:
            run.model.stats.update(buf["radii"], g, use_abs=run.args.absgrad)
        if sized or overflowed:                                         # K = ceil(1.25 x the largest D seen), at most 2^30
            cap["K"] = min(1 << 30, -(-5 * cap["max_D"] // 4))
        out.append((l_v, a_v, p_v, None, dxi))                           # (dxi: the re-run's, never the overflowed frame's)
    if sized:
        cap["n"] = n
    return out


def exchange_gradients(run, n, n_batch, arena, payloads):
    """Between "views done" and adam_update: this rank's summed gradient arena (None: it had no view) and its views' SH payloads
    become the batch-mean gradient that every rank applies.  Returns optimizer.adam_update's (grads, sh_views, sh_scale): factored,
    the payloads of all ranks' views, each rank padded with zero payloads to the same count (None, None once they are more than
    one kernel call takes: the SH gradient is then rebuilt in chunks); --dense-sh, the all-reduced dense arena."""
    dev, world, factored = run.dev, run.world, run.factored
    per_rank = -(-n_batch // world)                                     # views per rank, rounded up
    if arena is None:
        arena = torch.zeros(gsr.dist.arena_size(n, small=factored), device=dev)
    while factored and len(payloads) < per_rank:                        # ranks with a view less gather a zero payload
        payloads.append(torch.zeros(3 * n + 4, device=dev))
    if world != n_batch:
        arena.mul_(world / n_batch)                                     # mean over the batch after the /world of the average
    if not factored:
        if world > 1:
            gsr.dist.reduce_gradients(arena, world, average=True)
        return gsr.dist.arena_views(arena, n), None, None
    if world == 1:
        sh_views = payloads                                             # nothing to exchange: the Adam kernel takes the list as it is
    else:
        sh_views = gsr.dist.exchange_factored(arena, torch.stack(payloads).view(-1), average=True).view(world * per_rank, 3 * n + 4)
    grads = gsr.dist.small_arena_views(arena, n)
    grads["dL_dshs"] = None
    sh_scale = 1.0 / n_batch
    if len(sh_views) > gsr.dist.MAX_VIEWS_PER_CALL:                     # more views than one kernel call takes: rebuild in chunks
        grads["dL_dshs"] = gsr.dist.sh_gradients_from_views(run.model.params["positions"], torch.stack(list(sh_views)), 3, scale=sh_scale)
        sh_views, sh_scale = None, None
    return grads, sh_views, sh_scale


def density_control(run, it, n):
    """The reference's adaptive density control on the step's gradients (train.py:1060), its record and stdout line, and the 3D
    filter of the point set it leaves."""
    args, model = run.args, run.model
    if (run.screen_stats and run.world > 1 and it > args.densify_from and it < args.densify_until and it % args.densify_interval == 0):
        gsr.dist.reduce_densify_stats(model.stats, run.world)           # once per density-control call: every rank marks the same rows
    log = model.densification_and_pruning(it)
    if log["cloned"] or log["split"] or log["pruned"] or log["opacity_reset"] or log["prune_skipped"]:
        run.density_log.append({"iteration": it, "cloned": log["cloned"], "split": log["split"], "split_removed": log["split_removed"],
                                "pruned": log["pruned"], "prune_skipped": log["prune_skipped"], "opacity_reset": log["opacity_reset"],
                                "points": model.num_points})
    if args.filter_3d:
        if model.num_points != n or log["cloned"] or log["split"] or log["pruned"]:
            recompute_filter(run, it, "density_control")
        elif log["opacity_reset"]:
            recompute_filter(run, it, "opacity_reset")
        elif it >= args.densify_until and it % args.filter_3d_interval == 0:
            recompute_filter(run, it, "interval")
    if run.rank == 0 and (log["cloned"] or log["split"] or log["pruned"] or log["opacity_reset"]):
        print(f"iter {it:5d}  densify: +{log['cloned']} cloned, {log['split']} split, -{log['pruned']} pruned"
              f"{', opacity reset' if log['opacity_reset'] else ''} -> {model.num_points} points")


def print_loss(run, it, mine):
    """The iteration's loss line: one read of the curves' slots (a wait, hence --print-interval)"""
    args = run.args
    scale = mean_divisor(run, mine[0]) if len(mine) == 1 else None      # (one view: the slots hold sums)
    if run.dssim:                                                       # the combined loss (one read of both slots)
        l1_v, ssim_v = torch.stack([run.loss_hist[it], run.ssim_hist[it]]).tolist()
        l1_v, ssim_v = (l1_v / scale, ssim_v * 3.0 / scale) if scale is not None else (l1_v, ssim_v)
        shown = (1.0 - args.lambda_dssim) * l1_v + args.lambda_dssim * (1.0 - ssim_v)
    else:
        shown = float(run.loss_hist[it].item()) / (scale if scale is not None else 1.0)
    print(f"iter {it:5d}  loss {shown:.6f}", flush=True)


def train_step(run, it):
    """One iteration: this rank's views of the batch, the gradient exchange, Adam, density control, and what rank 0 writes."""
    args, model, dev, world, rank = run.args, run.model, run.dev, run.world, run.rank
    P, n = model.params, model.num_points
    assert not args.filter_3d or run.mode_kw["filter_3d"].shape[0] == n          # never a filter of another point set
    batch = run.rng.choice(len(run.views.cams), size=args.views_per_step, replace=False)
    mine = [int(batch[i]) for i in gsr.dist.views_for_rank(len(batch), rank, world)]
    alone = len(mine) == 1
    arena, loss_acc, payloads = None, (torch.zeros(1, device=dev) if len(mine) > 1 else None), []
    if args.capacity:
        done = capacity_views(run, it, mine, n)
    else:
        # a rank with several views renders them on separate streams (one view's sort chain under another's blend kernels) and
        # then sums them in view order, exactly as the serial loop does
        streams = run.streams_many if (args.view_streams > 1 or (args.view_streams == 0 and n >= (1 << 17))) else run.streams_few
        done = streams.map(lambda v: train_view(run, it, v, alone), mine)
    for v, (l_v, a_v, p_v, _, dxi) in zip(mine, done):
        if dxi is not None:                                             # --optimize-poses: one step per view, from the frame that counted
            pose_step(run, v, dxi)
        if len(mine) > 1:
            loss_acc += l_v
        arena = a_v if arena is None else arena.add_(a_v)
        if run.factored:
            payloads.append(p_v)
    grads, sh_views, sh_scale = exchange_gradients(run, n, len(batch), arena, payloads)
    lrs = {k: s.get_lr(it, args.iterations) for k, s in run.sched.items()}
    model.grads = gsr.optimizer.grads_from_backward(grads)              # train.py:1047-1051
    gsr.optimizer.adam_update(P, model.grads, model.adam_m, model.adam_v, lrs, iteration=it, sh_views=sh_views, sh_degree=3, sh_scale=sh_scale)
    if len(mine) > 1:
        run.loss_hist[it] = loss_acc[0] / len(mine)
        if run.dssim:
            run.ssim_hist[it] = sum(run.ssim_of[v] for v in mine)[0] / len(mine)
    elif alone:
        run.view_of.append(mine[0])                                     # written by the loss kernel as a SUM: scaled once, at the end
    density_control(run, it, n)
    if rank == 0 and args.output and (it % args.save_interval == 0 or it == args.iterations - 1):
        where = os.path.join(args.output, "point_cloud", f"iteration_{it}")
        gsr.point_cloud.save_ply(model.params, os.path.join(where, "point_cloud.ply"), model.num_points, filter_3d=run.mode_kw.get("filter_3d"))
        if run.expo is not None:                                        # the matrices beside the PLY
            with open(os.path.join(where, "exposure.json"), "w") as f:
                json.dump(run.expo.state_dict(), f)
    if rank == 0 and (it % args.print_interval == 0 or it == args.iterations - 1):
        print_loss(run, it, mine)


def rescale_curves(run):
    """After the last step: with one view per rank and step the curves' slots hold sums (mean_divisor): one division for each curve."""
    if run.per_rank_views != 1:
        return
    full = len(run.view_of) == run.loss_hist.numel()                    # (weighted sums: each iteration by its view's 3 M_v)
    scale = mean_divisor(run, run.view_of) if full else run.views.sum_scale
    run.loss_hist /= scale
    if run.dssim:
        run.ssim_hist /= scale / 3.0                                    # ... and sums of per-pixel SSIM


def main(argv=None):
    args = parse_args(argv)
    cloud = check_args(args)
    dev, rank, world = open_device(args)
    views = load_views(args, dev)
    P, init_info = init_params(args, dev, cloud)
    run = new_run(args, dev, rank, world, views, P, init_info)
    if args.filter_3d:
        recompute_filter(run, -1, "start")
    torch.cuda.synchronize(dev)
    t_start = time.perf_counter()
    for it in range(args.iterations):
        train_step(run, it)
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - t_start
    rescale_curves(run)
    if rank == 0:
        finish(run, wall)
        if args.mesh_out:                                               # the model's surface from its training views (extract_mesh.py)
            from extract_mesh import mesh_from_model
            mesh_from_model(gsr, run.model.params, run.views.cams, args.mesh_out, bg=run.bg, mode_kw=run.mode_kw, resolution=args.mesh_resolution,
                            min_weight=args.mesh_min_weight, alpha_min=args.normal_alpha_min, depth_mode=args.mesh_depth)


if __name__ == "__main__":
    main()
