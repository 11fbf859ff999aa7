#!/usr/bin/env python3
"""Time the depth-distortion stage (include/gsr_distortion.h) on a bench config (C3: 1 M Gaussians, 800 x 800; C0: the reference
trainer's initial 5 000 points): distortion.render_distortion with and without the forward's block masks, and backward() without and
with dL_ddistortion, through Python (device events over --calls calls, host marshalling and launches included).  One JSON line.
    python tools/distortion_bench.py [--config C3] [--calls 20] [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/distortion_bench.py --config C3 --calls 5 --reps 1
Under rocprofv3 --kernel-trace (a run of its own: no counters, no other tracing) the times of distortion_kernel<false> (forward) and
<true> (backward) stand beside blend_forward_kernel's and blend_backward_splat_kernel's from the same trace.  GSR_LIB=path/to/libgsr_hip.so
times another build."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
gsr = importlib.import_module("3dgs-native_amd")


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
    ap.add_argument("--config", default="C3", choices=["C0", "C2", "C3"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "distortion_bench needs the GPU"
    from conftest import backward_kwargs, render_kwargs
    dev = torch.device("cuda", 0)
    cfg = dict(gsr.scenes.CONFIGS[args.config])
    W, H = cfg.pop("width"), cfg.pop("height")
    if "init_scale" in cfg:     # C0: the reference trainer's initial point set
        ip = gsr.densify.init_gaussian_params(cfg["n"], cfg["init_scale"], dev)
        sc = {"means": ip["positions"].cpu().numpy(), "shs": ip["shs"].cpu().numpy().reshape(-1, 16, 3),
              "opacities": ip["opacities"].cpu().numpy().reshape(-1, 1), "scales": ip["scales"].cpu().numpy(), "rotations": ip["rotations"].cpu().numpy()}
    else:
        sc = gsr.scenes.synthetic_scene(cfg["n"], cfg["scale_median"], cfg["scale_sigma"], cfg["seed"])
    cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    kw = render_kwargs(sc, cam, width=W, height=H)
    kw.update({k: torch.as_tensor(np.ascontiguousarray(v)).to(dev) for k, v in kw.items() if k in ("means3D", "opacity", "scales", "rotations", "sh")})
    sc_t = {"means": kw["means3D"], "opacities": kw["opacity"], "scales": kw["scales"], "rotations": kw["rotations"], "shs": kw["sh"]}
    render = lambda: gsr.render_gaussians(**kw)
    buf = render()[2]
    out = (torch.empty((H, W), device=dev), torch.empty((H, W, 4), device=dev))
    dist, mom = gsr.distortion.render_distortion(buf, H, W, out=out)
    loss, g = gsr.loss.distortion_loss_and_gradients(dist, None, 100.0)
    dpix = torch.randn((H, W, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(0)) / (H * W * 3)
    bkw = backward_kwargs(sc_t, cam, kw, buf, dpix)
    fns = {"render_gaussians_ms": render,
           "render_distortion_ms": lambda: gsr.distortion.render_distortion(buf, H, W, out=out),
           "render_distortion_no_masks_ms": lambda: gsr.distortion.render_distortion(buf, H, W, out=out, use_block_masks=False),
           "backward_ms": lambda: gsr.backward(**bkw),
           "backward_with_distortion_ms": lambda: gsr.backward(**bkw, dL_ddistortion=g, distortion_moments=mom)}
    med = lambda v: sorted(v)[len(v) // 2]
    rec = {"config": args.config, "N": int(cfg["n"]), "D": int(buf["point_list"].shape[0]), "W": W, "H": H, "lib": os.path.basename(gsr._lib.LIB_PATH),
           "distortion_mean": float(dist.mean()), "loss": float(loss)}
    for name, fn in fns.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        rec[name] = round(med([timed(fn, args.calls) for _ in range(args.reps)]), 4)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
