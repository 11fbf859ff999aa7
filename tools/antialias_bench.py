#!/usr/bin/env python3
"""Time the classic against the antialiased mode (include/gsr_antialias.h) at a bench config (default C3: 800 x 800, 1 M Gaussians):
the `preprocess` and `geom_bwd` stages (the library's stage events, gsr_stage_timing) and the whole forward + backward step (device
events over --calls steps), the two modes alternating, --reps times; one JSON line with the medians and the ratios.
    python tools/antialias_bench.py [--config C3] [--calls 20] [--reps 7]
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
gsr = importlib.import_module("3dgs-native_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "antialias_bench needs the GPU"
    from conftest import backward_kwargs, render_kwargs
    cfg = dict(gsr.scenes.CONFIGS[args.config])
    W, H = cfg.pop("width"), cfg.pop("height")
    if "init_scale" in cfg:     # C0 / C2i: the reference trainer's initial point set
        ip = gsr.densify.init_gaussian_params(cfg["n"], cfg["init_scale"], torch.device("cuda", 0))
        sc = {"means": ip["positions"].cpu().numpy(), "shs": ip["shs"].cpu().numpy().reshape(-1, 16, 3),
              "opacities": ip["opacities"].cpu().numpy().reshape(-1, 1), "scales": ip["scales"].cpu().numpy(), "rotations": ip["rotations"].cpu().numpy()}
    else:
        sc = gsr.scenes.synthetic_scene(cfg["n"], cfg["scale_median"], cfg["scale_sigma"], cfg["seed"])
    cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    kw = render_kwargs(sc, cam, width=W, height=H)
    dev = torch.device("cuda", 0)
    kw.update({k: torch.as_tensor(np.ascontiguousarray(v)).to(dev) for k, v in kw.items() if k in ("means3D", "opacity", "scales", "rotations", "sh")})
    kw["opacity"] = kw["opacity"].reshape(-1)
    sc_t = {"means": kw["means3D"], "opacities": kw["opacity"], "scales": kw["scales"], "rotations": kw["rotations"], "shs": kw["sh"]}
    g = torch.Generator(device="cuda").manual_seed(0)
    dpix = torch.randn((H, W, 3), device="cuda", generator=g) / (H * W * 3)
    modes = {"classic": {}, "antialiased": {"rasterize_mode": "antialiased"}}

    def step(mode):
        _, _, buf = gsr.render_gaussians(**kw, **mode)
        gsr.backward(**backward_kwargs(sc_t, cam, kw, buf, dpix), **mode)
        return buf

    D = {}
    for name, mode in modes.items():                                   # warm up both
        for _ in range(3):
            D[name] = int(step(mode)["point_list"].shape[0])
    torch.cuda.synchronize()
    times = {k: [] for k in modes}
    stages = {k: {"preprocess": [], "geom_bwd": []} for k in modes}
    for _ in range(args.reps):
        for name, mode in modes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                step(mode)
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / args.calls)
            gsr._lib.stage_timing(True, args.calls)                    # the stages in a pass of their own (event records are not free)
            for _ in range(args.calls):
                step(mode)
            torch.cuda.synchronize()
            st, n = gsr._lib.stage_times()
            gsr._lib.stage_timing(False)
            if n:
                for k in stages[name]:
                    stages[name][k].append(st[k])
    med = lambda v: sorted(v)[len(v) // 2] if v else None
    step_med = {k: med(v) for k, v in times.items()}
    stage_med = {k: {s: med(v) for s, v in d.items()} for k, d in stages.items()}
    ratio = lambda a, b: round(a / b, 4) if a and b else None
    print(json.dumps({"config": args.config, "D": D, "lib": os.path.basename(gsr._lib.LIB_PATH),
                      "step_ms_median": {k: round(v, 4) for k, v in step_med.items()},
                      "step_ms_all": {k: [round(x, 4) for x in v] for k, v in times.items()},
                      "stage_us_median": {k: {s: round(1e3 * v, 2) if v else None for s, v in d.items()} for k, d in stage_med.items()},
                      "antialiased_over_classic": {"step": ratio(step_med["antialiased"], step_med["classic"]),
                                                   "preprocess": ratio(stage_med["antialiased"]["preprocess"], stage_med["classic"]["preprocess"]),
                                                   "geom_bwd": ratio(stage_med["antialiased"]["geom_bwd"], stage_med["classic"]["geom_bwd"])}}), flush=True)


if __name__ == "__main__":
    main()
