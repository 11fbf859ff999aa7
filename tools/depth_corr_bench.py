#!/usr/bin/env python3
"""Time the Pearson-correlation depth loss (include/gsr_depth_corr.h): loss.depth_corr_loss_and_gradients alone at 800 x 800 and
1920 x 1080, with and without the gradient, against loss.depth_loss_and_gradients (gsr_depth_loss_grad, the masked L1) on the same
box in the same process (device events over --calls calls, host marshalling and launch included), with the bytes the three launches
move and the rate that makes; and one trainer iteration with --depth-loss l1 and --depth-loss pearson (examples/train.py in
hidden-scene mode, --lambda-depth 1 --depth-noise 1, for --trainer-iterations iterations, alternating, --trainer-reps times; 0 = skip);
one JSON line.
    python tools/depth_corr_bench.py [--calls 200] [--reps 7] [--trainer-iterations 1000] [--trainer-reps 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/depth_corr_bench.py --calls-only --calls 20 --reps 1 --sizes 800x800
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

# per pixel, with a mask: the sums pass reads r, t, m; the gradient pass reads them again and writes grad.  The masked L1 reads the
# three and writes grad, once.
SUMS_BYTES, GRAD_BYTES, L1_BYTES = 12, 16, 16
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
    """ms per iteration of examples/train.py on the hidden scene at its default size with the depth term as the masked L1 and as
    1 - rho, alternating: each run is a fresh process (the GPU is idle here while it runs) and reports its own iterations/s."""
    ms = {"l1": [], "pearson": []}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(reps):
            for name in ms:
                log = os.path.join(tmp, name + ".jsonl")
                subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--views", "8", "--iterations", str(iterations),
                                "--lambda-depth", "1.0", "--depth-noise", "1", "--depth-loss", name, "--print-interval", "100000", "--log", log],
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
    assert torch.cuda.is_available(), "depth_corr_bench needs the GPU"
    dev = torch.device("cuda", 0)
    L = gsr.loss
    med = lambda v: sorted(v)[len(v) // 2]
    gen = torch.Generator(device="cuda").manual_seed(0)
    sizes = {}
    for W, H in (tuple(int(x) for x in wh.split("x")) for wh in args.sizes.split(",")):
        r = torch.rand((H, W), device=dev, generator=gen) * 2.0
        t = 0.6 * r + 0.3 + 0.15 * torch.randn((H, W), device=dev, generator=gen)
        m = (torch.rand((H, W), device=dev, generator=gen) > 0.2).float()
        loss, fit = torch.empty(1, device=dev), torch.empty(4, device=dev)
        fns = {"pearson_us": lambda: L.depth_corr_loss_and_gradients(r, t, m, 0.1, loss_out=loss, fit_out=fit),
               "pearson_loss_only_us": lambda: L.depth_corr_loss_and_gradients(r, t, m, 0.1, want_grad=False, loss_out=loss, fit_out=fit),
               "pearson_no_mask_us": lambda: L.depth_corr_loss_and_gradients(r, t, None, 0.1, loss_out=loss, fit_out=fit),
               "l1_us": lambda: L.depth_loss_and_gradients(r, t, m, 0.1, loss_out=loss)}
        calls = {}
        for name, fn in fns.items():
            fn()
            calls[name] = 1e3 * med([timed(fn, args.calls) for _ in range(args.reps)])
        P = W * H
        sizes[f"{W}x{H}"] = {"calls_us": {k: round(v, 2) for k, v in calls.items()},
                             "bytes_MB": {"pearson": round((SUMS_BYTES + GRAD_BYTES) * P * 1e-6, 2), "l1": round(L1_BYTES * P * 1e-6, 2)},
                             "call_rate_TB_s": {"pearson": round((SUMS_BYTES + GRAD_BYTES) * P / calls["pearson_us"] * 1e-6, 3),
                                                "l1": round(L1_BYTES * P / calls["l1_us"] * 1e-6, 3)},
                             "pearson_over_l1": round(calls["pearson_us"] / calls["l1_us"], 3)}
    # (a call's time is the larger of its kernels and the Python that marshals and enqueues them: see the kernel trace for the kernels)
    trainer = {}
    if not args.calls_only and args.trainer_iterations > 0:
        torch.cuda.synchronize()
        ms = trainer_iteration(args.trainer_iterations, args.trainer_reps)
        trainer = {"trainer_iterations": args.trainer_iterations, "trainer_ms_per_iteration_median": {k: round(med(v), 4) for k, v in ms.items()},
                   "trainer_ms_per_iteration_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                   "trainer_iterations_per_s_median": {k: round(1e3 / med(v), 1) for k, v in ms.items()},
                   "pearson_over_l1_trainer": round(med(ms["pearson"]) / med(ms["l1"]), 4)}
    print(json.dumps({"lib": os.path.basename(gsr._lib.LIB_PATH), "sizes": sizes, **trainer}), flush=True)


if __name__ == "__main__":
    main()
