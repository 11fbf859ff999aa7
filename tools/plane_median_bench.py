#!/usr/bin/env python3
"""Time the plane depth under the median rule (include/gsr_plane_median.h) on a bench config (C3: 1 M Gaussians, 800 x 800; C0: the
reference trainer's initial 5 000 points): plane_depth.render_plane_median_depth with and without the forward's block masks,
median_depth.render_median_depth and plane_depth.render_plane_depth beside it (the two kernels it is made of),
plane_depth.plane_median_depth_backward, and the three calls of plane_depth.plane_median_gradients together, through Python (device
events over --calls calls, host marshalling and launches included).  One JSON line per config, with the share of the Gaussians that take
the plane branch and the share of the chosen pixels whose value differs from the centre median's.  --flatten R shrinks every
Gaussian's smallest scale to R times itself first, as tools/plane_depth_bench.py does: the configs' own scales are round three times in
four and would time the fallback.
    python tools/plane_median_bench.py [--config C0 C3] [--calls 20] [--repeats 5] [--flatten 0.3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/plane_median_bench.py --config C3 --calls 5 --repeats 1
Under rocprofv3 --kernel-trace (a run of its own: no counters, no other tracing) the times of plane_median_kernel and
plane_median_backward_kernel stand beside median_depth_kernel's, median_depth_backward_kernel's, plane_depth_kernel<false>'s and
blend_forward_kernel's from the same trace.  GSR_LIB=path/to/libgsr_hip.so times another build."""
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
    from conftest import render_kwargs
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
    P = {"positions": kw["means3D"], "scales": kw["scales"], "rotations": kw["rotations"]}
    render = lambda: gsr.render_gaussians(**kw)
    buf = render()[2]
    N = int(cfg["n"])
    pdm, md = gsr.plane_depth, gsr.median_depth
    n = gsr.normal_render.gaussian_normals(kw["scales"], kw["rotations"], kw["means3D"], cam)
    slopes = pdm.plane_slopes(n, kw["scales"], kw["means3D"], cam)
    out = (torch.empty((H, W), device=dev), torch.empty((H, W), dtype=torch.int32, device=dev))
    out_c = (torch.empty((H, W), device=dev), torch.empty((H, W), dtype=torch.int32, device=dev))
    pd_out, mom = torch.empty((H, W), device=dev), torch.empty((N, 3), device=dev)
    med, contrib = (t.clone() for t in pdm.render_plane_median_depth(slopes, buf, H, W))
    centre = md.render_median_depth(buf, H, W)
    assert torch.equal(contrib, centre[1]), "the contributor does not depend on the slopes"
    g = torch.full((H, W), 1.0 / (W * H), device=dev)
    dmean, drot = torch.zeros((N, 3), device=dev), torch.zeros((N, 4), device=dev)
    grads = {"dL_dmean3D": dmean, "dL_drot": drot}
    fns = {"render_gaussians_ms": render,
           "render_plane_median_depth_ms": lambda: pdm.render_plane_median_depth(slopes, buf, H, W, out=out),
           "render_plane_median_depth_no_masks_ms": lambda: pdm.render_plane_median_depth(slopes, buf, H, W, out=out, use_block_masks=False),
           "render_median_depth_ms": lambda: md.render_median_depth(buf, H, W, out=out_c),
           "render_plane_depth_ms": lambda: pdm.render_plane_depth(slopes, buf, H, W, out=pd_out),
           "plane_median_depth_backward_ms": lambda: pdm.plane_median_depth_backward(g, contrib, slopes, buf, H, W, out=mom),
           "plane_median_gradients_ms": lambda: pdm.plane_median_gradients(P, cam, buf, g, contrib, slopes, n, grads=grads)}
    mid = lambda v: sorted(v)[len(v) // 2]
    chosen = contrib > 0
    rec = {"config": config, "N": N, "D": int(buf["point_list"].shape[0]), "W": W, "H": H, "lib": os.path.basename(gsr._lib.LIB_PATH), "flatten": flatten,
           "plane_branch_share": float((slopes != 0).any(1).double().mean()), "chosen_share": float(chosen.double().mean()),
           "differs_from_centre_median_share": float((med != centre[0])[chosen].double().mean()) if bool(chosen.any()) else 0.0}
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
    assert torch.cuda.is_available(), "plane_median_bench needs the GPU"
    for config in args.config:
        bench(gsr, config, args.calls, args.repeats, None if args.flatten == 1.0 else args.flatten)


if __name__ == "__main__":
    main()
