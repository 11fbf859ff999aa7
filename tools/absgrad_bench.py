#!/usr/bin/env python3
"""Time backward() at a bench config (default C3: 800 x 800, 1 M Gaussians; C0 is the other one recorded) without and with
absgrad=True (include/gsr_densify_stats.h, GSR_BWD_ABSGRAD), and the statistics update on its own: the two backward calls
alternate, each timed with device events over --calls calls, --reps times; then --calls statistics updates per repetition, signed
and absolute columns alternating.  One JSON line with the medians, the ratio, and the bytes one update moves.
    python tools/absgrad_bench.py [--config C3] [--calls 20] [--reps 7]
Kernel times (blend_bwd: default, AUX and ABS instantiations; densify_stats_update_kernel): run it under
rocprofv3 --kernel-trace --stats in a run of its own; SQ_INSTS_VALU in a counter run of its own.  GSR_LIB=path/to/libgsr_hip.so times
another build (--no-abs for a build that lacks the flag, e.g. the parent commit's)."""
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
    ap.add_argument("--no-abs", action="store_true", help="time the plain backward only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "absgrad_bench needs the GPU"
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
    sc_t = {"means": kw["means3D"], "opacities": kw["opacity"], "scales": kw["scales"], "rotations": kw["rotations"], "shs": kw["sh"]}
    _, _, buf = gsr.render_gaussians(**kw)
    g = torch.Generator(device="cuda").manual_seed(0)
    dpix = torch.randn((H, W, 3), device="cuda", generator=g) / (H * W * 3)
    bkw = backward_kwargs(sc_t, cam, kw, buf, dpix)
    runs = {"plain": {}} if args.no_abs else {"plain": {}, "absgrad": {"absgrad": True}}
    for extra in runs.values():                                        # warm up both
        for _ in range(3):
            out = gsr.backward(**bkw, **extra)
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.reps):
        for name, extra in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                out = gsr.backward(**bkw, **extra)
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / args.calls)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    rec = {"config": args.config, "N": int(cfg["n"]), "D": int(buf["point_list"].shape[0]), "lib": os.path.basename(gsr._lib.LIB_PATH),
           "backward_ms_median": {k: round(v, 4) for k, v in med.items()},
           "backward_ms_all": {k: [round(x, 4) for x in v] for k, v in times.items()}}
    if not args.no_abs:
        rec["absgrad_over_plain"] = round(med["absgrad"] / med["plain"], 4)
        n = int(cfg["n"])
        stats = gsr.densify.DensifyStats(n, dev)
        upd = {"signed": [], "abs": []}
        for _ in range(3):
            stats.update(buf["radii"], out, use_abs=True)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name in upd:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.calls):
                    stats.update(buf["radii"], out, use_abs=name == "abs")
                b.record()
                b.synchronize()
                upd[name].append(1e3 * a.elapsed_time(b) / args.calls)
        visible = int((buf["radii"] > 0).sum().item())
        # per Gaussian 4 B of radii; per visible one 8 B of its record (one 32-byte sector of the 64-byte row as the memory
        # system fetches it) and three 4-byte read-modify-writes (read + write)
        rec["stats_update_us_median"] = {k: round(sorted(v)[len(v) // 2], 2) for k, v in upd.items()}
        rec["stats_update_us_all"] = {k: [round(x, 2) for x in v] for k, v in upd.items()}
        rec["stats_update_visible"] = visible
        rec["stats_update_bytes"] = {"algorithmic": 4 * n + visible * (8 + 3 * 8), "sector_granular": 4 * n + visible * (32 + 3 * 8)}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
