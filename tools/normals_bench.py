#!/usr/bin/env python3
"""Time the normals stage (include/gsr_normals.h): normals.normals_from_depth, normals.normals_from_depth_backward and
loss.normal_loss_and_gradients (with the gradient, loss only, without a mask) at 800 x 800 and 1920 x 1080, against
loss.depth_loss_and_gradients (gsr_depth_loss_grad, the masked L1) on the same box in the same process (device events over --calls
calls, host marshalling and launch included), with the bytes each call has to move and the rate that makes; and one trainer iteration
with and without --lambda-normal (examples/train.py in hidden-scene mode for --trainer-iterations iterations, alternating,
--trainer-reps times; 0 = skip); one JSON line.
    python tools/normals_bench.py [--calls 200] [--reps 7] [--trainer-iterations 1000] [--trainer-reps 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/normals_bench.py --calls-only --calls 20 --reps 1 --sizes 800x800
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

# unique bytes per pixel: the loss reads Dinv, final_T, the target and the mask and writes gD and gA; the VJP reads dL/dn for the
# target and no mask; the forward reads the two images and writes normals and valid; the masked L1 reads three images and writes one
BYTES = {"loss_us": 32, "loss_no_mask_us": 28, "loss_only_us": 24, "vjp_us": 28, "forward_us": 24, "l1_us": 16}
SIZES = ((800, 800), (1920, 1080))
LAMBDA_NORMAL = "0.05"


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def trainer_iteration(iterations, reps):
    """ms per iteration of examples/train.py on the hidden scene at its default size without and with the normal term, alternating:
    each run is a fresh process (the GPU is idle here while it runs) and reports its own iterations/s."""
    ms = {"plain": [], "normal": []}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(reps):
            for name in ms:
                log = os.path.join(tmp, name + ".jsonl")
                extra = ["--lambda-normal", LAMBDA_NORMAL] if name == "normal" else []
                subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--views", "8", "--iterations", str(iterations),
                                "--print-interval", "100000", "--log", log, *extra], check=True, stdout=subprocess.DEVNULL, timeout=600)
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
    assert torch.cuda.is_available(), "normals_bench needs the GPU"
    dev = torch.device("cuda", 0)
    L, N = gsr.loss, gsr.normals
    med = lambda v: sorted(v)[len(v) // 2]
    gen = torch.Generator(device="cuda").manual_seed(0)
    sizes = {}
    for W, H in (tuple(int(x) for x in wh.split("x")) for wh in args.sizes.split(",")):
        cam = {"tan_fovx": 0.5, "tan_fovy": 0.5 * H / W, "width": W, "height": H}
        x = torch.linspace(0, 6, W, device=dev)[None, :]
        y = torch.linspace(0, 5, H, device=dev)[:, None]
        T = 0.3 * torch.rand((H, W), device=dev, generator=gen)
        T[torch.rand((H, W), device=dev, generator=gen) < 0.05] = 0.9          # 5 % of the pixels below alpha_min
        D = ((1.0 - T) / (3.0 + 0.4 * torch.sin(x) * torch.cos(y))).contiguous()
        n, valid = N.normals_from_depth(D, T, cam)
        t = (n + 0.2 * torch.randn((H, W, 3), device=dev, generator=gen)).contiguous()
        m = (torch.rand((H, W), device=dev, generator=gen) > 0.2).float()
        g = torch.randn((H, W, 3), device=dev, generator=gen)
        sums, slot = torch.empty(2, device=dev), torch.empty(1, device=dev)
        fns = {"loss_us": lambda: L.normal_loss_and_gradients(D, T, t, cam, m, 0.05, loss_out=sums),
               "loss_no_mask_us": lambda: L.normal_loss_and_gradients(D, T, t, cam, None, 0.05, loss_out=sums),
               "loss_only_us": lambda: L.normal_loss_and_gradients(D, T, t, cam, m, 0.05, want_grad=False, loss_out=sums),
               "vjp_us": lambda: N.normals_from_depth_backward(g, D, T, cam),
               "forward_us": lambda: N.normals_from_depth(D, T, cam),
               "l1_us": lambda: L.depth_loss_and_gradients(D, T, m, 0.1, loss_out=slot)}
        calls = {}
        for name, fn in fns.items():
            fn()
            calls[name] = 1e3 * med([timed(fn, args.calls) for _ in range(args.reps)])
        P = W * H
        sizes[f"{W}x{H}"] = {"valid_share": round(float(valid.mean().item()), 4), "calls_us": {k: round(v, 2) for k, v in calls.items()},
                             "bytes_MB": {k: round(b * P * 1e-6, 2) for k, b in BYTES.items()},
                             "call_rate_TB_s": {k: round(b * P / calls[k] * 1e-6, 3) for k, b in BYTES.items()},
                             "loss_over_l1": round(calls["loss_us"] / calls["l1_us"], 3)}
    # (a call's time is the larger of its kernels and the Python that marshals and enqueues them: see the kernel trace for the kernels)
    trainer = {}
    if not args.calls_only and args.trainer_iterations > 0:
        torch.cuda.synchronize()
        ms = trainer_iteration(args.trainer_iterations, args.trainer_reps)
        trainer = {"trainer_iterations": args.trainer_iterations, "trainer_ms_per_iteration_median": {k: round(med(v), 4) for k, v in ms.items()},
                   "trainer_ms_per_iteration_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                   "trainer_iterations_per_s_median": {k: round(1e3 / med(v), 1) for k, v in ms.items()},
                   "normal_over_plain_trainer": round(med(ms["normal"]) / med(ms["plain"]), 4)}
    print(json.dumps({"lib": os.path.basename(gsr._lib.LIB_PATH), "sizes": sizes, **trainer}), flush=True)


if __name__ == "__main__":
    main()
