#!/usr/bin/env python3
"""Time N-channel feature rendering (include/gsr_features.h) on a BASELINE config (default C3: 1 M Gaussians, 800 x 800): the forward
and the backward for C = 3, 16 and 64 over one rendered frame, through features.render_features / render_features_backward (device
events over --calls calls, host marshalling and launches included), with and without the forward's block masks, and the frame's
live pair counts for scale.  One JSON line.
    python tools/features_bench.py [--config C3] [--calls 20] [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/features_bench.py --calls 5 --reps 1 --channels 16 --masks-only
Under rocprofv3 --kernel-trace the kernel times of features_kernel stand beside blend_forward_kernel's from the same trace (the frame
is rendered --calls times too, for that).  GSR_LIB=path/to/libgsr_hip.so times another build."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gsr = importlib.import_module("3dgs-native_amd")
feat = importlib.import_module("3dgs-native_amd.features")


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C2", "C3", "C5"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--channels", default="3,16,64")
    ap.add_argument("--masks-only", action="store_true", help="time only the calls that use the forward's block masks (for a kernel trace of one path)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "features_bench needs the GPU"
    dev = torch.device("cuda", 0)
    cfg = gsr.scenes.CONFIGS[args.config]
    W, H = cfg["width"], cfg["height"]
    sc = gsr.scenes.synthetic_scene(cfg["n"], cfg["scale_median"], cfg["scale_sigma"], cfg["seed"])
    t = {k: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32), device=dev) for k, v in sc.items()}
    cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)

    def render():
        return gsr.render_gaussians(background=np.zeros(3, np.float32), means3D=t["means"], colors=None, opacity=t["opacities"], scales=t["scales"],
                                    rotations=t["rotations"], scale_modifier=1.0, viewmatrix=cam["world_to_camera"], projmatrix=cam["full_proj_matrix"],
                                    tan_fovx=cam["tan_fovx"], tan_fovy=cam["tan_fovy"], image_height=H, image_width=W, sh=t["shs"].reshape(-1, 3), degree=3,
                                    campos=cam["camera_center"], prefiltered=False, antialiasing=False, clamped=True)
    buf = render()[2]
    N, D = t["means"].shape[0], int(buf["point_list"].shape[0])
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"config": args.config, "N": N, "D": D, "W": W, "H": H, "lib": os.path.basename(gsr._lib.LIB_PATH)}
    render()
    out["render_gaussians_ms"] = round(med([timed(render, args.calls) for _ in range(args.reps)]), 4)
    gen = torch.Generator(device=dev).manual_seed(0)
    for C in (int(c) for c in args.channels.split(",")):
        F = torch.rand((N, C), device=dev, generator=gen) * 2 - 1
        G = torch.rand((H, W, C), device=dev, generator=gen) * 2 - 1
        o, dF = torch.empty((H, W, C), device=dev), torch.empty((N, C), device=dev)
        fns = {"forward_ms": lambda: feat.render_features(F, buf, H, W, out=o),
               "forward_no_masks_ms": lambda: feat.render_features(F, buf, H, W, out=o, use_block_masks=False),
               "backward_ms": lambda: feat.render_features_backward(G, buf, H, W, out=dF),
               "backward_no_masks_ms": lambda: feat.render_features_backward(G, buf, H, W, out=dF, use_block_masks=False)}
        if args.masks_only:
            fns = {k: v for k, v in fns.items() if "no_masks" not in k}
        row = {}
        for name, fn in fns.items():
            fn()
            row[name] = round(med([timed(fn, args.calls) for _ in range(args.reps)]), 4)
        Fr = F.clone().requires_grad_(True)

        def step():
            Fr.grad = None
            (feat.rasterize_features(Fr, buf, H, W) * G).sum().backward()
        if not args.masks_only:
            step()
            row["autograd_step_ms"] = round(med([timed(step, args.calls) for _ in range(args.reps)]), 4)
        row["rows_touched"] = int((dF.abs().amax(1) > 0).sum())
        out[f"C{C}"] = row
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
