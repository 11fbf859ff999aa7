#!/usr/bin/env python3
"""Time the plane-depth stage (include/gsr_plane_depth.h) on a bench config (C3: 1 M Gaussians, 800 x 800; C0: the reference trainer's
initial 5 000 points): plane_depth.plane_slopes, plane_depth.render_plane_depth with and without the forward's block masks,
normal_render.render_normals and distortion.render_distortion beside it (the neighbours on the same walk), and backward() without and
with dL_dplane_depth, through Python (device events over --calls calls, host marshalling and launches included).  One JSON line per
config, with the share of the Gaussians that take the plane branch.  --flatten R shrinks every Gaussian's smallest scale to R times
itself first: the configs' own scales are round three times in four and would time the fallback.
    python tools/plane_depth_bench.py [--config C0 C3] [--calls 20] [--repeats 5] [--flatten 0.3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/plane_depth_bench.py --config C3 --calls 5 --repeats 1
Under rocprofv3 --kernel-trace (a run of its own: no counters, no other tracing) the times of plane_slopes_kernel<false|true> and
plane_depth_kernel<false|true> stand beside normal_render_kernel's, distortion_kernel's and blend_forward_kernel's from the same trace.
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


def bench(gsr, config, calls, repeats, flatten):
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
    if flatten is not None:
        s = np.array(sc["scales"], np.float32)
        s[np.arange(len(s)), s.argmin(1)] *= np.float32(flatten)
        sc["scales"] = s
    cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    kw = render_kwargs(sc, cam, width=W, height=H)
    kw.update({k: torch.as_tensor(np.ascontiguousarray(v)).to(dev) for k, v in kw.items() if k in ("means3D", "opacity", "scales", "rotations", "sh")})
    sc_t = {"means": kw["means3D"], "opacities": kw["opacity"], "scales": kw["scales"], "rotations": kw["rotations"], "shs": kw["sh"]}
    render = lambda: gsr.render_gaussians(**kw)
    buf = render()[2]
    N = int(cfg["n"])
    n = gsr.normal_render.gaussian_normals(kw["scales"], kw["rotations"], kw["means3D"], cam)
    s_out, pd_out = torch.empty((N, 2), device=dev), torch.empty((H, W), device=dev)
    n_out, dout = torch.empty((H, W, 3), device=dev), (torch.empty((H, W), device=dev), torch.empty((H, W, 4), device=dev))
    slopes = gsr.plane_depth.plane_slopes(n, kw["scales"], kw["means3D"], cam, out=s_out)
    pd = gsr.plane_depth.render_plane_depth(slopes, buf, H, W).clone()
    g = torch.full((H, W), 1.0 / (W * H), device=dev)
    dpix = torch.randn((H, W, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(0)) / (H * W * 3)
    bkw = backward_kwargs(sc_t, cam, kw, buf, dpix)
    plane_kw = dict(dL_dplane_depth=g, plane_slopes=slopes, plane_depth_image=pd, gaussian_normals=n)
    fns = {"render_gaussians_ms": render,
           "plane_slopes_ms": lambda: gsr.plane_depth.plane_slopes(n, kw["scales"], kw["means3D"], cam, out=s_out),
           "render_plane_depth_ms": lambda: gsr.plane_depth.render_plane_depth(slopes, buf, H, W, out=pd_out),
           "render_plane_depth_no_masks_ms": lambda: gsr.plane_depth.render_plane_depth(slopes, buf, H, W, out=pd_out, use_block_masks=False),
           "render_normals_ms": lambda: gsr.normal_render.render_normals(n, buf, H, W, out=n_out),
           "render_distortion_ms": lambda: gsr.distortion.render_distortion(buf, H, W, out=dout),
           "backward_ms": lambda: gsr.backward(**bkw),
           "backward_with_plane_depth_ms": lambda: gsr.backward(**bkw, **plane_kw),
           "backward_with_plane_depth_no_param_grad_ms": lambda: gsr.backward(**bkw, **plane_kw, plane_param_grad=False)}
    mid = lambda v: sorted(v)[len(v) // 2]
    rec = {"config": config, "N": N, "D": int(buf["point_list"].shape[0]), "W": W, "H": H, "lib": os.path.basename(gsr._lib.LIB_PATH), "flatten": flatten,
           "plane_branch_share": float((slopes != 0).any(1).double().mean())}
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
    ap.add_argument("--flatten", type=float, default=0.3, metavar="R", help="shrink every Gaussian's smallest scale to R times itself (1: as drawn)")
    args = ap.parse_args()
    if not 0.0 < args.flatten <= 1.0:
        ap.error("--flatten must lie in (0, 1]")
    gsr = importlib.import_module("3dgs-native_amd")
    assert torch.cuda.is_available(), "plane_depth_bench needs the GPU"
    for config in args.config:
        bench(gsr, config, args.calls, args.repeats, None if args.flatten == 1.0 else args.flatten)


if __name__ == "__main__":
    main()
