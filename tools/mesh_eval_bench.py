"""
Times of the mesh-evaluation stage (include/gsr_mesh_eval.h) on the MI355X, device events around whole calls:

    nearest   100 k x 100 k and 1 M x 1 M on two sets sampled from concentric spheres a small offset apart (the real workload: both
              sets lie on surfaces), and 1 M x 1 M uniform in a cube
    sampler   1 M triangles -> about 1 M samples (count, the host read, emit)
    for scale gsr_knn at the same N, and torch.cdist + min at 20 k x 20 k

    python tools/mesh_eval_bench.py [--repeats 5] [--json OUT] [--only CASE] [--once]

--only CASE --once runs one call of one case and nothing else: what a kernel trace of its own wants.  One JSON line per case.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def sphere_points(n, radius, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    p = torch.randn((n, 3), generator=g, device=dev)
    return (p / p.norm(dim=1, keepdim=True) * radius).contiguous()


def cube_points(n, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand((n, 3), generator=g, device=dev) * 2.6 - 1.3).contiguous()


def timed(fn, repeats, warmup=1):
    """Median, minimum and maximum milliseconds of fn() over `repeats` calls, by device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None, metavar="OUT")
    ap.add_argument("--only", default=None, metavar="CASE")
    ap.add_argument("--once", action="store_true", help="one untimed call per case (for a kernel trace)")
    args = ap.parse_args()
    gsr = importlib.import_module("3dgs-native_amd")
    me, knn = gsr.mesh_eval, gsr.knn
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def spheres(n):
        return sphere_points(n, 1.0, 1, dev), sphere_points(n, 1.01, 2, dev)

    def soup(t):
        g = torch.Generator(device=dev).manual_seed(3)
        centre = torch.rand((t, 1, 3), generator=g, device=dev) * 2 - 1
        return (centre + 0.002 * torch.randn((t, 3, 3), generator=g, device=dev)).contiguous()

    cases = {}
    for n in (100_000, 1_000_000):
        cases[f"nearest_spheres_{n}"] = (lambda n=n: spheres(n), lambda d: me.nearest(d[0], d[1]))
    cases["nearest_cube_1000000"] = (lambda: (cube_points(1_000_000, 4, dev), cube_points(1_000_000, 5, dev)), lambda d: me.nearest(d[0], d[1]))
    cases["nearest_spheres_1000000_cap"] = (lambda: spheres(1_000_000), lambda d: me.nearest(d[0], d[1], max_dist=0.05))
    cases["sample_1000000_triangles"] = (lambda: soup(1_000_000), lambda d: me.sample_mesh(d, samples=1_000_000))
    for n in (100_000, 1_000_000):
        cases[f"knn_sphere_{n}"] = (lambda n=n: sphere_points(n, 1.0, 1, dev), lambda d: knn.knn(d))
    cases["knn_cube_1000000"] = (lambda: cube_points(1_000_000, 4, dev), lambda d: knn.knn(d))
    cases["cdist_min_20000"] = (lambda: spheres(20_000), lambda d: torch.cdist(d[0], d[1]).min(dim=1))
    if args.only is not None and args.only not in cases:
        raise SystemExit(f"--only: one of {', '.join(cases)}")
    out = []
    for name, (make, call) in cases.items():
        if args.only is not None and name != args.only:
            continue
        data = make()
        torch.cuda.synchronize()
        if args.once:
            call(data)
            torch.cuda.synchronize()
            rec = {"case": name, "once": True}
        else:
            rec = {"case": name, **timed(lambda: call(data), args.repeats)}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del data
    if args.json:
        with open(args.json, "w") as f:
            for rec in out:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
