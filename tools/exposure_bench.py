#!/usr/bin/env python3
"""Time per-view exposure compensation (include/gsr_exposure.h): the three calls of exposure.py alone at 800 x 800 and 1920 x 1080
(device events over --calls calls, host marshalling and launch included; the backward in place, as the trainer calls it), with the
bytes the two image kernels move and the rate that makes; and one trainer iteration with and without --optimize-exposure
(examples/train.py on data/lego for --trainer-iterations iterations, alternating, --trainer-reps times; 0 = skip); one JSON line.
    python tools/exposure_bench.py [--calls 200] [--reps 7] [--trainer-iterations 1000] [--trainer-reps 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/exposure_bench.py --calls-only --calls 20 --reps 1 --sizes 800x800
--calls-only stops after the calls: under rocprofv3 --kernel-trace that gives the kernels alone, at one size with --sizes.
GSR_LIB=path/to/libgsr_hip.so times another build."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gsr = importlib.import_module("3dgs-native_amd")

APPLY_BYTES, BACKWARD_BYTES = 24, 36        # per pixel: image in, image out; image + gradient in, gradient out
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
    """ms per iteration of examples/train.py on the committed Lego views, without and with --optimize-exposure, alternating: each run
    is a fresh process (the GPU is idle here while it runs) and reports its own iterations/s."""
    ms = {"plain": [], "optimize_exposure": []}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(reps):
            for name, extra in (("plain", []), ("optimize_exposure", ["--optimize-exposure"])):
                log = os.path.join(tmp, name + ".jsonl")
                subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--dataset", os.path.join(ROOT, "data", "lego"), "--views", "8",
                                "--iterations", str(iterations), "--print-interval", "1000", "--log", log, *extra],
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
    assert torch.cuda.is_available(), "exposure_bench needs the GPU"
    dev = torch.device("cuda", 0)
    X = gsr.exposure
    med = lambda v: sorted(v)[len(v) // 2]
    gen = torch.Generator(device="cuda").manual_seed(0)
    model = X.ExposureModel(8, dev)
    sizes = {}
    for W, H in (tuple(int(x) for x in wh.split("x")) for wh in args.sizes.split(",")):
        img = torch.rand((H, W, 3), device=dev, generator=gen)
        g = torch.randn((H, W, 3), device=dev, generator=gen) / (H * W * 3)
        out, dE = torch.empty_like(img), torch.empty(12, device=dev)
        E = model.matrix(3)
        fns = {"apply_us": lambda: X.apply_exposure(img, E, out=out), "backward_us": lambda: X.exposure_backward(img, E, g, out=g, dE_out=dE),
               "backward_sums_only_us": lambda: X.exposure_backward(img, E, g, want_image_grad=False, dE_out=dE)}
        if not sizes:
            fns["adam_us"] = lambda: model.step(3, dE, 0.0)
        calls = {}
        for name, fn in fns.items():
            fn()
            calls[name] = 1e3 * med([timed(fn, args.calls) for _ in range(args.reps)])
        P = W * H
        sizes[f"{W}x{H}"] = {"calls_us": {k: round(v, 2) for k, v in calls.items()},
                             "stream_rate_TB_s": {"apply": round(APPLY_BYTES * P / calls["apply_us"] * 1e-6, 3),
                                                  "backward": round(BACKWARD_BYTES * P / calls["backward_us"] * 1e-6, 3)}}
    # (a call's time is the larger of its kernels and the Python that marshals and enqueues them: see the kernel trace for the kernels)
    trainer = {}
    if not args.calls_only and args.trainer_iterations > 0:
        torch.cuda.synchronize()
        ms = trainer_iteration(args.trainer_iterations, args.trainer_reps)
        trainer = {"trainer_iterations": args.trainer_iterations, "trainer_ms_per_iteration_median": {k: round(med(v), 4) for k, v in ms.items()},
                   "trainer_ms_per_iteration_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                   "trainer_iterations_per_s_median": {k: round(1e3 / med(v), 1) for k, v in ms.items()},
                   "exposure_over_plain_trainer": round(med(ms["optimize_exposure"]) / med(ms["plain"]), 4)}
    print(json.dumps({"lib": os.path.basename(gsr._lib.LIB_PATH), "sizes": sizes, **trainer}), flush=True)


if __name__ == "__main__":
    main()
