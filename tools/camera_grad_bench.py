#!/usr/bin/env python3
"""Time backward() at a bench config (default C3: 800 x 800, 1 M Gaussians) without and with camera_grad=True
(include/gsr_camera_grads.h): the two calls alternate, each timed with device events over --calls calls, --reps
times; one JSON line with the medians and the ratio.
    python tools/camera_grad_bench.py [--config C3] [--calls 20] [--reps 7]
Kernel times (camera_partials_kernel, camera_finish_kernel): run it under rocprofv3 --kernel-trace --stats in a run of
its own.  GSR_LIB=path/to/libgsr_hip.so times another build."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "camera_grad_bench needs the GPU"
    from conftest import backward_kwargs, render_kwargs
    cfg = dict(gsr.scenes.CONFIGS[args.config])
    W, H = cfg.pop("width"), cfg.pop("height")
    sc = gsr.scenes.synthetic_scene(cfg["n"], cfg["scale_median"], cfg["scale_sigma"], cfg["seed"])
    cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    kw = render_kwargs(sc, cam, width=W, height=H)
    dev = torch.device("cuda", 0)
    kw.update({k: torch.as_tensor(np.ascontiguousarray(v)).to(dev) for k, v in kw.items() if k in ("means3D", "opacity", "scales", "rotations", "sh")})
    sc_t = {"means": kw["means3D"], "opacities": kw["opacity"], "scales": kw["scales"], "rotations": kw["rotations"], "shs": kw["sh"]}
    _, _, buf = gsr.render_gaussians(**kw)
    g = torch.Generator(device="cuda").manual_seed(0)
    dpix = torch.randn((H, W, 3), device="cuda", generator=g) / (H * W * 3)
    bkw = backward_kwargs(sc_t, cam, kw, buf, dpix)
    runs = {"plain": {}, "camera": {"camera_grad": True}}
    for extra in runs.values():                                        # warm up both
        for _ in range(3):
            gsr.backward(**bkw, **extra)
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.reps):
        for name, extra in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                gsr.backward(**bkw, **extra)
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / args.calls)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(json.dumps({"config": args.config, "D": int(buf["point_list"].shape[0]), "lib": os.path.basename(gsr._lib.LIB_PATH),
                      "backward_ms_median": {k: round(v, 4) for k, v in med.items()},
                      "backward_ms_all": {k: [round(x, 4) for x in v] for k, v in times.items()},
                      "camera_over_plain": round(med["camera"] / med["plain"], 4),
                      "camera_added_ms": round(med["camera"] - med["plain"], 4)}), flush=True)


if __name__ == "__main__":
    main()
