#!/usr/bin/env python3
"""Time the colour loss with and without per-pixel weights (include/gsr_weighted_loss.h): the calls of loss.py at 800 x 800 and
1920 x 1080 (device events over --calls calls, host marshalling and launch included), weighted against unweighted, for the D-SSIM
loss, the L1 loss and the weight total; and one trainer iteration with and without an all-ones --mask-dir (examples/train.py on
data/lego with --lambda-dssim 0.2 for --trainer-iterations iterations, alternating, --trainer-reps times; 0 = skip); one JSON line.
    python tools/weighted_loss_bench.py [--calls 200] [--reps 7] [--trainer-iterations 1000] [--trainer-reps 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/weighted_loss_bench.py --calls-only --calls 20 --reps 1 --sizes 800x800
--calls-only stops after the calls: under rocprofv3 --kernel-trace that gives the kernels alone, at one size with --sizes.
The estimate the kernels are held against: the two weighted D-SSIM passes read one H W plane of weights each on top of the roughly
125 bytes per pixel of the unweighted call (80 MB at 800 x 800), i.e. +8 bytes per pixel, under +10 %.
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
gsr = importlib.import_module("3dgs-native_amd")

SIZES = ((800, 800), (1920, 1080))


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def trainer_iteration(iterations, reps):
    """ms per iteration of examples/train.py on the committed Lego views, without and with an all-ones --mask-dir, alternating: each
    run is a fresh process (the GPU is idle here while it runs) and reports its own iterations/s."""
    from PIL import Image
    ms = {"plain": [], "all_ones_mask": []}
    with tempfile.TemporaryDirectory() as tmp:
        masks = os.path.join(tmp, "masks")
        os.makedirs(masks)
        for k in range(8):
            Image.fromarray(np.full((800, 800), 255, np.uint8)).save(os.path.join(masks, f"r_{k}.png"))
        for _ in range(reps):
            for name, extra in (("plain", []), ("all_ones_mask", ["--mask-dir", masks])):
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--sizes", default=",".join(f"{w}x{h}" for w, h in SIZES), help="image sizes WxH, separated by commas")
    ap.add_argument("--trainer-iterations", type=int, default=1000)
    ap.add_argument("--trainer-reps", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "weighted_loss_bench needs the GPU"
    dev = torch.device("cuda", 0)
    loss = gsr.loss
    med = lambda v: sorted(v)[len(v) // 2]
    gen = torch.Generator(device="cuda").manual_seed(0)
    sizes = {}
    for W, H in (tuple(int(x) for x in wh.split("x")) for wh in args.sizes.split(",")):
        t = torch.rand((H, W, 3), device=dev, generator=gen)
        r = (t + 0.1 * torch.randn((H, W, 3), device=dev, generator=gen)).clamp(0, 1)
        m = (torch.rand((H, W), device=dev, generator=gen) > 0.3).float()
        pw = loss.PixelWeights(m)
        fns = {"dssim_us": lambda: loss.l1_dssim_loss_and_gradients(r, t, 0.2), "weighted_dssim_us": lambda: loss.l1_dssim_loss_and_gradients(r, t, 0.2, weights=pw),
               "l1_us": lambda: loss.l1_loss_and_gradients(r, t), "weighted_l1_us": lambda: loss.l1_loss_and_gradients(r, t, weights=pw),
               "weight_total_us": lambda: loss.PixelWeights(m)}
        calls = {}
        for name, fn in fns.items():
            fn()
            calls[name] = 1e3 * med([timed(fn, args.calls) for _ in range(args.reps)])
        sizes[f"{W}x{H}"] = {"calls_us": {k: round(v, 2) for k, v in calls.items()},
                             "weighted_over_unweighted": {"dssim": round(calls["weighted_dssim_us"] / calls["dssim_us"], 4),
                                                          "l1": round(calls["weighted_l1_us"] / calls["l1_us"], 4)}}
    # (a call's time is the larger of its kernels and the Python that marshals and enqueues them: see the kernel trace for the kernels)
    trainer = {}
    if not args.calls_only and args.trainer_iterations > 0:
        torch.cuda.synchronize()
        ms = trainer_iteration(args.trainer_iterations, args.trainer_reps)
        trainer = {"trainer_iterations": args.trainer_iterations, "trainer_ms_per_iteration_median": {k: round(med(v), 4) for k, v in ms.items()},
                   "trainer_ms_per_iteration_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                   "trainer_iterations_per_s_median": {k: round(1e3 / med(v), 1) for k, v in ms.items()},
                   "mask_over_plain_trainer": round(med(ms["all_ones_mask"]) / med(ms["plain"]), 4)}
    print(json.dumps({"lib": os.path.basename(gsr._lib.LIB_PATH), "sizes": sizes, **trainer}), flush=True)


if __name__ == "__main__":
    main()
