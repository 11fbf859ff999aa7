#!/usr/bin/env python3
"""Time gsr_l1_dssim_loss_grad (include/gsr_loss.h) per call with device events, at 800 x 800 and 1920 x 1080, and state the bytes
the call must move and the rate that implies.  One JSON line per size.
    python tools/dssim_bench.py [--calls 200] [--reps 5] [--no-grad]
GSR_LIB=path/to/libgsr_hip.so times another build (A/B on one box).  Kernel times: run it under rocprofv3 --kernel-trace --stats
in a run of its own."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gsr = importlib.import_module("3dgs-native_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=5, help="timed windows per size (the median is reported)")
    ap.add_argument("--no-grad", action="store_true", help="the two sums alone (pixel_grad = NULL)")
    ap.add_argument("--window", default="gaussian", choices=["gaussian", "reference"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dssim_bench needs the GPU"
    L = gsr._lib.lib()
    for W, H in ((800, 800), (1920, 1080)):
        g = torch.Generator(device="cuda").manual_seed(0)
        t = torch.rand((H, W, 3), device="cuda", generator=g)
        r = (t + 0.1 * torch.randn((H, W, 3), device="cuda", generator=g)).clamp(0, 1)
        l1, ss = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
        for _ in range(20):                                           # warm up: code objects, the workspace cache
            gsr.loss.l1_dssim_loss_and_gradients(r, t, 0.2, args.window, not args.no_grad, l1, ss)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                gsr.loss.l1_dssim_loss_and_gradients(r, t, 0.2, args.window, not args.no_grad, l1, ss)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / args.calls)
        us = sorted(times)[len(times) // 2]
        n = H * W * 3 * 4                                             # bytes of one float32 image
        compulsory = 2 * n + (0 if args.no_grad else n)               # both images in, the gradient out
        ws = int(L.gsr_dssim_workspace_bytes(W, H))
        planes = 9 * H * W * 4 if ws >= 9 * H * W * 4 else 0          # the two-kernel join writes and reads 9 floats per pixel
        moved = compulsory + (2 * planes if not args.no_grad else 0)
        print(json.dumps({"W": W, "H": H, "lib": os.path.basename(gsr._lib.LIB_PATH), "grad": not args.no_grad, "window": args.window,
                          "us_per_call_median": round(us, 2), "us_per_call_all": [round(x, 2) for x in times],
                          "compulsory_MB": round(compulsory / 1e6, 2), "with_workspace_MB": round(moved / 1e6, 2),
                          "compulsory_TBps": round(compulsory / us / 1e6, 3), "with_workspace_TBps": round(moved / us / 1e6, 3)}), flush=True)


if __name__ == "__main__":
    main()
