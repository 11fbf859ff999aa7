#!/usr/bin/env python3
"""
Lift 2D label maps onto a frozen splat model with N-channel feature rendering (3dgs-native_amd/features.py).

A hidden seeded scene gives every Gaussian a label from the octant of its position (8 classes, one-hot features).  The targets are
the label maps of 8 orbit views, rendered with render_features() from the hidden one-hot features.  The example then fits a feature
array F (N, 8) from zero on the frozen geometry -- rasterize_features() inside a torch optimiser, one view per iteration -- and
reports the loss curve and the pixel accuracy of argmax(F rendered) against the true label map on a ninth view, between two of the
training views, as one JSON line.

    python examples/fit_features.py [--size 256] [--iterations 400] [--gaussians 4000] [--lr 0.05] [--seed 0] [--out DIR]

--out DIR writes PNGs of three per-Gaussian attributes rendered as images on the ninth view: normals.png (the shortest axis of
every Gaussian, 0.5 + 0.5 n), log_scale.png (mean log scale, normalised over the scene) and labels.png (the fitted labels as a
palette).
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PALETTE = np.array([[230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200], [245, 130, 48], [145, 30, 180], [70, 240, 240], [240, 50, 230]],
                   np.float32) / 255.0
N_VIEWS, N_CLASSES = 8, 8


def shortest_axis(scales, rotations):
    """(N, 3): the rotation-matrix column of each Gaussian's smallest scale; rotations are (x, y, z, w)."""
    x, y, z, w = (rotations[:, i].astype(np.float64) for i in range(4))
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)      # (N, 3, 3)
    return R[np.arange(len(x)), :, scales.argmin(1)].astype(np.float32)


def save_png(path, image):
    from PIL import Image
    arr = np.clip(image.detach().cpu().numpy(), 0.0, 1.0)
    Image.fromarray((arr * 255.0 + 0.5).astype(np.uint8)).save(path)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.strip().splitlines()[0])
    ap.add_argument("--size", type=int, default=256, help="image side in pixels")
    ap.add_argument("--iterations", type=int, default=400, help="optimiser steps, one view each")
    ap.add_argument("--gaussians", type=int, default=4000, help="Gaussians of the hidden scene")
    ap.add_argument("--lr", type=float, default=0.05, help="Adam learning rate")
    ap.add_argument("--seed", type=int, default=0, help="seed of the hidden scene")
    ap.add_argument("--out", default=None, metavar="DIR", help="write normals.png, log_scale.png and labels.png of the ninth view here")
    a = ap.parse_args(argv)
    if a.iterations < 1:
        ap.error("--iterations must be at least 1")
    if a.size < 16 or a.gaussians < 8:
        ap.error("--size must be at least 16 and --gaussians at least 8")

    gsr = importlib.import_module("3dgs-native_amd")
    feat = importlib.import_module("3dgs-native_amd.features")
    dev = torch.device("cuda", torch.cuda.current_device())
    S = a.size
    sc = gsr.scenes.synthetic_scene(a.gaussians, 0.05, 0.6, a.seed)
    N = sc["means"].shape[0]
    tens = {k: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32), device=dev) for k, v in sc.items()}
    P = {"positions": tens["means"], "scales": tens["scales"], "rotations": tens["rotations"], "opacities": tens["opacities"],
         "shs": tens["shs"].reshape(-1, 3)}
    labels = (sc["means"][:, 0] > 0).astype(np.int64) + 2 * (sc["means"][:, 1] > 0) + 4 * (sc["means"][:, 2] > 0)
    hidden = torch.nn.functional.one_hot(torch.as_tensor(labels, device=dev), N_CLASSES).to(torch.float32).contiguous()

    def frame(k):
        cam = gsr.cameras.nerf_camera(gsr.scenes.orbit_pose(k, N_VIEWS), S, S, gsr.scenes.LEGO_CAMERA_ANGLE_X)
        return gsr.render_view(P, cam, np.zeros(3, np.float32))[2]

    frames = [frame(k) for k in range(N_VIEWS)]                                  # the frozen geometry: drawn once per view
    targets = [feat.render_features(hidden, b, S, S) for b in frames]
    F = torch.zeros(N, N_CLASSES, device=dev, requires_grad=True)
    opt = torch.optim.Adam([F], lr=a.lr)
    losses = []
    for it in range(a.iterations):
        v = it % N_VIEWS
        opt.zero_grad(set_to_none=True)
        loss = torch.mean((feat.rasterize_features(F, frames[v], S, S) - targets[v]) ** 2)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(x) for x in torch.stack(losses).cpu()]

    held = frame(0.5)                                                            # the ninth view, between views 0 and 1
    with torch.no_grad():
        want, got = feat.render_features(hidden, held, S, S), feat.render_features(F.detach().contiguous(), held, S, S)
        covered = held["final_Ts"] < 0.5
        accuracy = float((want.argmax(2) == got.argmax(2))[covered].float().mean()) if bool(covered.any()) else float("nan")
    step = max(1, a.iterations // 10)
    summary = dict(example="fit_features", size=S, gaussians=N, iterations=a.iterations, lr=a.lr, seed=a.seed, views=N_VIEWS, classes=N_CLASSES,
                   first_loss=losses[0], final_loss=losses[-1], loss_curve=[[i, losses[i]] for i in range(0, a.iterations, step)],
                   heldout_covered_pixels=int(covered.sum()), heldout_accuracy=accuracy)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        normal = torch.as_tensor(0.5 + 0.5 * shortest_axis(sc["scales"], sc["rotations"]), device=dev).contiguous()
        save_png(os.path.join(a.out, "normals.png"), feat.render_features(normal, held, S, S))
        ls = np.log(sc["scales"]).mean(1)
        ls = ((ls - ls.min()) / max(float(ls.max() - ls.min()), 1e-12)).astype(np.float32)
        save_png(os.path.join(a.out, "log_scale.png"), feat.render_features(torch.as_tensor(ls[:, None], device=dev).contiguous(), held, S, S).expand(S, S, 3))
        pal = torch.as_tensor(PALETTE, device=dev)[F.detach().argmax(1)].contiguous()
        save_png(os.path.join(a.out, "labels.png"), feat.render_features(pal, held, S, S))
        summary["out"] = a.out
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
