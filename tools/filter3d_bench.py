#!/usr/bin/env python3
"""Time the 3D smoothing filter (include/gsr_filter3d.h) at a bench config (default C3: 800 x 800, 1 M Gaussians): the three calls
of filter3d.py (device events over --calls calls, host packing and launch included; from_views at V = 8 and V = 100 orbit cameras),
with the bytes the two streams move and the rate that makes; the whole forward + backward step with and without the `filter_3d`
keyword, alternating, --reps times; and one trainer iteration with and without --filter-3d (examples/train.py on data/lego for
--trainer-iterations iterations, alternating, --trainer-reps times; 0 = skip); one JSON line with the medians.
    python tools/filter3d_bench.py [--config C3] [--calls 50] [--reps 7] [--trainer-iterations 2000] [--trainer-reps 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/filter3d_bench.py --calls-only --calls 20 --reps 1
--calls-only stops after the three calls: under rocprofv3 --kernel-trace that gives the three kernels alone.
GSR_LIB=path/to/libgsr_hip.so times another build."""
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

APPLY_BYTES, BACKWARD_BYTES = 36, 52        # per Gaussian: scales + opacity + filter in, (cotangents in,) scales + opacity out


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def trainer_iteration(iterations, reps):
    """ms per iteration of examples/train.py on the committed Lego views, without and with --filter-3d, alternating: each run is a
    fresh process (the GPU is idle here while it runs) and reports its own iterations/s, density control and recomputations included."""
    ms = {"plain": [], "filter_3d": []}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(reps):
            for name, extra in (("plain", []), ("filter_3d", ["--filter-3d"])):
                log = os.path.join(tmp, name + ".jsonl")
                subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--dataset", os.path.join(ROOT, "data", "lego"), "--views", "8",
                                "--iterations", str(iterations), "--lambda-dssim", "0.2", "--print-interval", "1000", "--log", log, *extra],
                               check=True, stdout=subprocess.DEVNULL, timeout=600)
                with open(log) as fh:
                    summary = [r for r in map(json.loads, fh) if r["record"] == "summary"][0]
                ms[name].append(1e3 / summary["iterations_per_s"])
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--trainer-iterations", type=int, default=2000)
    ap.add_argument("--trainer-reps", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "filter3d_bench needs the GPU"
    from conftest import backward_kwargs, render_kwargs
    cfg = dict(gsr.scenes.CONFIGS[args.config])
    W, H = cfg.pop("width"), cfg.pop("height")
    dev = torch.device("cuda", 0)
    if "init_scale" in cfg:     # C0 / C2i: the reference trainer's initial point set
        ip = gsr.densify.init_gaussian_params(cfg["n"], cfg["init_scale"], dev)
        sc = {"means": ip["positions"].cpu().numpy(), "shs": ip["shs"].cpu().numpy().reshape(-1, 16, 3),
              "opacities": ip["opacities"].cpu().numpy().reshape(-1, 1), "scales": ip["scales"].cpu().numpy(), "rotations": ip["rotations"].cpu().numpy()}
    else:
        sc = gsr.scenes.synthetic_scene(cfg["n"], cfg["scale_median"], cfg["scale_sigma"], cfg["seed"])
    N = sc["means"].shape[0]
    cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    kw = render_kwargs(sc, cam, width=W, height=H)
    kw.update({k: torch.as_tensor(np.ascontiguousarray(v)).to(dev) for k, v in kw.items() if k in ("means3D", "opacity", "scales", "rotations", "sh")})
    kw["opacity"] = kw["opacity"].reshape(-1)
    sc_t = {"means": kw["means3D"], "opacities": kw["opacity"], "scales": kw["scales"], "rotations": kw["rotations"], "shs": kw["sh"]}
    dpix = torch.randn((H, W, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)) / (H * W * 3)
    med = lambda v: sorted(v)[len(v) // 2]
    F = gsr.filter3d
    orbit = lambda V: [gsr.cameras.nerf_camera(gsr.scenes.orbit_pose(k, V), W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X) for k in range(V)]
    out = torch.empty(N, device=dev)
    calls = {}
    for V in (8, 100):
        cams = orbit(V)
        F.compute_filter_3d(kw["means3D"], cams, out=out)
        calls[f"from_views_V{V}_us"] = 1e3 * med([timed(lambda: F.compute_filter_3d(kw["means3D"], cams, out=out), args.calls) for _ in range(args.reps)])
    f = F.compute_filter_3d(kw["means3D"], orbit(8))
    so = (torch.empty_like(kw["scales"]), torch.empty_like(kw["opacity"]))
    gs, go = torch.randn_like(kw["scales"]), torch.randn_like(kw["opacity"])
    F.apply_filter_3d(kw["scales"], kw["opacity"], f, out=so), F.filter_3d_backward(kw["scales"], kw["opacity"], f, gs, go, out=so)
    calls["apply_us"] = 1e3 * med([timed(lambda: F.apply_filter_3d(kw["scales"], kw["opacity"], f, out=so), args.calls) for _ in range(args.reps)])
    calls["backward_us"] = 1e3 * med([timed(lambda: F.filter_3d_backward(kw["scales"], kw["opacity"], f, gs, go, out=so), args.calls) for _ in range(args.reps)])
    # (a call's time is the larger of its kernels and the Python that packs the views and enqueues them)
    if args.calls_only:
        print(json.dumps({"config": args.config, "N": N, "lib": os.path.basename(gsr._lib.LIB_PATH), "calls_us": {k: round(v, 2) for k, v in calls.items()}}), flush=True)
        return
    rates = {"apply_TB_s": APPLY_BYTES * N / calls["apply_us"] * 1e-6, "backward_TB_s": BACKWARD_BYTES * N / calls["backward_us"] * 1e-6}
    modes = {"plain": {}, "filter_3d": {"filter_3d": f}}

    def step(mode):
        _, _, buf = gsr.render_gaussians(**kw, **mode)
        gsr.backward(**backward_kwargs(sc_t, cam, kw, buf, dpix), **mode)

    for mode in modes.values():
        for _ in range(3):
            step(mode)
    torch.cuda.synchronize()
    times = {k: [] for k in modes}
    for _ in range(args.reps):
        for name, mode in modes.items():
            times[name].append(timed(lambda: step(mode), max(1, args.calls // 2)))
    step_med = {k: med(v) for k, v in times.items()}
    trainer = {}
    if args.trainer_iterations > 0:
        torch.cuda.synchronize()
        ms = trainer_iteration(args.trainer_iterations, args.trainer_reps)
        trainer = {"trainer_iterations": args.trainer_iterations, "trainer_ms_per_iteration_median": {k: round(med(v), 4) for k, v in ms.items()},
                   "trainer_ms_per_iteration_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                   "filter_over_plain_trainer": round(med(ms["filter_3d"]) / med(ms["plain"]), 4)}
    print(json.dumps({"config": args.config, "N": N, "lib": os.path.basename(gsr._lib.LIB_PATH), "calls_us": {k: round(v, 2) for k, v in calls.items()},
                      "stream_rate": {k: round(v, 3) for k, v in rates.items()}, "step_ms_median": {k: round(v, 4) for k, v in step_med.items()},
                      "step_ms_all": {k: [round(x, 4) for x in v] for k, v in times.items()},
                      "filter_over_plain_step": round(step_med["filter_3d"] / step_med["plain"], 4), **trainer}), flush=True)


if __name__ == "__main__":
    main()
