#!/usr/bin/env python3
"""Time gsr_knn (include/gsr_knn.h) through knn.knn: uniform points in the reference's cube (-1.3, 1.3)^3 at 100 000 and 1 000 000,
and a clustered cloud of 1 000 000 (the three-component Gaussian mixture of tests/test_gpu_knn.py); device events over --calls
calls, host marshalling and launches included.  For scale, what a user would write today -- torch.cdist + topk -- at N = 20 000: its
distance matrix alone is 4 N^2 bytes, 1.6 GB there and 4 TB at 1 M, so it cannot run at the sizes above.  One JSON line.
    python tools/knn_bench.py [--calls 20] [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/knn_bench.py --calls-only --calls 5 --reps 1 --cases uniform_1000000
--calls-only skips the torch comparison: under rocprofv3 --kernel-trace that gives this feature's kernels alone, one case with --cases.
GSR_LIB=path/to/libgsr_hip.so times another build."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gsr = importlib.import_module("3dgs-native_amd")

CASES = ("uniform_100000", "uniform_1000000", "mixture_1000000")


def cloud(case, dev):
    kind, n = case.split("_")
    n = int(n)
    gen = torch.Generator(device=dev).manual_seed(0)
    if kind == "uniform":
        return torch.rand((n, 3), device=dev, generator=gen) * 2.6 - 1.3
    which = torch.randint(0, 3, (n,), device=dev, generator=gen)
    centre = torch.tensor([[0.0, 0.0, 0.0], [2.0, -1.0, 0.5], [-3.0, 4.0, 1.0]], device=dev)[which]
    sigma = torch.tensor([0.02, 0.3, 1.5], device=dev)[which][:, None]
    return (centre + torch.randn((n, 3), device=dev, generator=gen) * sigma).contiguous()


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--cdist-n", type=int, default=20000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "knn_bench needs the GPU"
    dev = torch.device("cuda", 0)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {}
    for case in args.cases.split(","):
        pts = cloud(case, dev)
        n = pts.shape[0]
        mean = torch.empty(n, device=dev)
        pair = (mean, torch.empty((n, 3), dtype=torch.int32, device=dev))
        fns = {"knn_ms": lambda: gsr.knn.knn(pts, out=mean), "knn_with_indices_ms": lambda: gsr.knn.knn(pts, want_indices=True, out=pair)}
        row = {}
        for name, fn in fns.items():
            fn()
            row[name] = round(med([timed(fn, args.calls) for _ in range(args.reps)]), 4)
        row["workspace_MB"] = round(gsr._lib.lib().gsr_knn_workspace_bytes(n) * 1e-6, 1)
        row["scale_min_median_max"] = [round(float(x), 5) for x in (lambda s: (s.min(), s.median(), s.max()))(torch.sqrt(mean))]
        out[case] = row
    if not args.calls_only:
        n = args.cdist_n
        pts = cloud(f"uniform_{n}", dev)

        def brute():
            d = torch.cdist(pts, pts)
            return (d.topk(4, dim=1, largest=False).values[:, 1:] ** 2).mean(dim=1)
        brute()
        ours = lambda: gsr.knn.knn(pts)
        ours()
        out[f"uniform_{n}"] = {"torch_cdist_topk_ms": round(med([timed(brute, 5) for _ in range(args.reps)]), 4),
                               "knn_ms": round(med([timed(ours, args.calls) for _ in range(args.reps)]), 4),
                               "cdist_matrix_GB": round(4 * n * n * 1e-9, 2)}
    print(json.dumps({"lib": os.path.basename(gsr._lib.LIB_PATH), "cases": out}), flush=True)


if __name__ == "__main__":
    main()
