#!/usr/bin/env python3
"""Time the median-depth stage (include/gsr_median_depth.h) on a bench config (C3: 1 M Gaussians, 800 x 800; C0: the reference
trainer's initial 5 000 points): median_depth.render_median_depth with and without the forward's block masks, distortion.render_distortion
beside it (the neighbour that walks every list to its end), and backward() without and with dL_dmedian_depth, through Python (device
events over --calls calls, host marshalling and launches included).  One JSON line per config, with what the early exit had to work
with: the share of the list entries inside n_contrib that lie at or before the median.
    python tools/median_depth_bench.py [--config C0 C3] [--calls 20] [--repeats 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/median_depth_bench.py --config C3 --calls 5 --repeats 1
Under rocprofv3 --kernel-trace (a run of its own: no counters, no other tracing) the times of median_depth_kernel and
median_depth_backward_kernel stand beside distortion_kernel<false>'s and blend_forward_kernel's from the same trace.
GSR_LIB=path/to/libgsr_hip.so times another build."""
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


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def bench(gsr, config, calls, repeats):
    from conftest import backward_kwargs, render_kwargs
    dev = torch.device("cuda", 0)
    cfg = dict(gsr.scenes.CONFIGS[config])
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
    out = (torch.empty((H, W), device=dev), torch.empty((H, W), dtype=torch.int32, device=dev))
    dout = (torch.empty((H, W), device=dev), torch.empty((H, W, 4), device=dev))
    med, contrib = gsr.median_depth.render_median_depth(buf, H, W, out=out)
    g = torch.full((H, W), 1.0 / (W * H), device=dev)
    dpix = torch.randn((H, W, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(0)) / (H * W * 3)
    bkw = backward_kwargs(sc_t, cam, kw, buf, dpix)
    fns = {"render_gaussians_ms": render,
           "render_median_depth_ms": lambda: gsr.median_depth.render_median_depth(buf, H, W, out=out),
           "render_median_depth_no_masks_ms": lambda: gsr.median_depth.render_median_depth(buf, H, W, out=out, use_block_masks=False),
           "render_distortion_ms": lambda: gsr.distortion.render_distortion(buf, H, W, out=dout),
           "backward_ms": lambda: gsr.backward(**bkw),
           "backward_with_median_depth_ms": lambda: gsr.backward(**bkw, dL_dmedian_depth=g, median_contributor=contrib)}
    mid = lambda v: sorted(v)[len(v) // 2]
    nc = buf["n_contrib"].reshape(H, W).double()
    rec = {"config": config, "N": int(cfg["n"]), "D": int(buf["point_list"].shape[0]), "W": W, "H": H, "lib": os.path.basename(gsr._lib.LIB_PATH),
           "pixels_with_a_median": float((contrib > 0).double().mean()), "median_position_mean": float(contrib.double().mean()),
           "n_contrib_mean": float(nc.mean()), "median_over_n_contrib": float(contrib.double().sum() / nc.sum().clamp(min=1.0))}
    for name, fn in fns.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        rec[name] = round(mid([timed(fn, calls) for _ in range(repeats)]), 4)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", nargs="+", default=["C0", "C3"], choices=["C0", "C2", "C3"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    gsr = importlib.import_module("3dgs-native_amd")
    assert torch.cuda.is_available(), "median_depth_bench needs the GPU"
    for config in args.config:
        bench(gsr, config, args.calls, args.repeats)


if __name__ == "__main__":
    main()
