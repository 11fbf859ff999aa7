#!/usr/bin/env python3
"""Time the normal-rendering stage (include/gsr_normal_render.h) on a bench config (C3: 1 M Gaussians, 800 x 800; C0: the reference
trainer's initial 5 000 points): the five calls through Python (device events over --calls calls, host marshalling and launches
included) beside features.render_features at C = 3 and backward() without and with the three keywords.  One JSON line.
    python tools/normal_render_bench.py [--config C3] [--calls 20] [--reps 5]
    python tools/normal_render_bench.py --trainer        (one trainer iteration at --size 100 --views 8, without and with the term)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/normal_render_bench.py --config C3 --calls 5 --reps 1
Under rocprofv3 --kernel-trace (a run of its own: no counters, no other tracing) the times of gaussian_normals_kernel,
normal_render_kernel<false> / <true> and consistency_kernel stand beside features_kernel's, blend_forward_kernel's and
blend_backward_splat_kernel's from the same trace.  GSR_LIB=path/to/libgsr_hip.so times another build."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile

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


def trainer_iterations():
    """ms per iteration of examples/train.py at --size 100 --views 8 over 300 iterations, without and with the term (fresh processes)."""
    out = {}
    for tag, extra in (("trainer_iteration_ms", []), ("trainer_iteration_with_term_ms", ["--lambda-normal-consistency", "0.05"])):
        with tempfile.TemporaryDirectory() as d:
            log = os.path.join(d, "log.jsonl")
            subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--size", "100", "--views", "8", "--iterations", "300",
                            "--log", log, "--print-interval", "1000", *extra], cwd=ROOT, check=True, capture_output=True, timeout=1200)
            for line in open(log):
                rec = json.loads(line)
                if rec["record"] == "summary":
                    out[tag] = round(1000.0 * rec["wall_s"] / rec["iterations"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C0", "C2", "C3"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trainer", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "normal_render_bench needs the GPU"
    if args.trainer:
        print(json.dumps(trainer_iterations()), flush=True)
        return
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
    image, depth, buf = render()
    depth, T = depth.reshape(H, W), buf["final_Ts"].reshape(H, W)
    nr = gsr.normal_render
    N = int(kw["means3D"].shape[0])
    n = torch.empty((N, 3), device=dev)
    normals = lambda: nr.gaussian_normals(kw["scales"], kw["rotations"], kw["means3D"], cam, out=n)
    normals()
    nimg = torch.empty((H, W, 3), device=dev)
    nr.render_normals(n, buf, H, W, out=nimg)
    sums, gN, gD, gA = gsr.loss.normal_consistency_loss_and_gradients(nimg, depth, T, cam, None, 0.05)
    drot = torch.zeros((N, 4), device=dev)
    dpix = torch.randn((H, W, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(0)) / (H * W * 3)
    bkw = backward_kwargs(sc_t, cam, kw, buf, dpix)
    triple = dict(dL_dnormal_image=gN, gaussian_normals=n, normal_image=nimg)
    fns = {"render_gaussians_ms": render,
           "gaussian_normals_ms": normals,
           "gaussian_normals_backward_ms": lambda: nr.gaussian_normals_backward(n, kw["scales"], kw["rotations"], kw["means3D"], cam, dL_drot=drot),
           "render_normals_ms": lambda: nr.render_normals(n, buf, H, W, out=nimg),
           "render_normals_no_masks_ms": lambda: nr.render_normals(n, buf, H, W, out=nimg, use_block_masks=False),
           "render_features_c3_ms": lambda: gsr.features.render_features(n, buf, H, W),
           "normal_consistency_loss_ms": lambda: gsr.loss.normal_consistency_loss_and_gradients(nimg, depth, T, cam, None, 0.05),
           "backward_ms": lambda: gsr.backward(**bkw),
           "backward_with_depth_images_ms": lambda: gsr.backward(**bkw, dL_ddepth_image=gD, dL_dalpha_image=gA),
           "backward_with_normals_ms": lambda: gsr.backward(**bkw, dL_ddepth_image=gD, dL_dalpha_image=gA, **triple)}
    med = lambda v: sorted(v)[len(v) // 2]
    s = sums.cpu().numpy()
    rec = {"config": args.config, "N": N, "D": int(buf["point_list"].shape[0]), "W": W, "H": H, "lib": os.path.basename(gsr._lib.LIB_PATH),
           "counted_pixels": float(s[1]), "mean_term": float(s[0] / s[1]) if s[1] > 0 else None}
    for name, fn in fns.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        rec[name] = round(med([timed(fn, args.calls) for _ in range(args.reps)]), 4)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
