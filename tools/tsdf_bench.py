#!/usr/bin/env python3
"""Time the TSDF stage (include/gsr_tsdf.h): integration of V views of 800 x 800 into a G^3 colour volume, batched
(TSDFVolume.integrate_views: 16 views per launch) against one call per view (TSDFVolume.integrate), and the triangle count and emit
of a sphere volume of the same size.  Times are device events around the Python calls (host marshalling and launch included; the
median of --reps repetitions); one JSON line.
    python tools/tsdf_bench.py [--sizes 256,512] [--views 8,100] [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/tsdf_bench.py --sizes 512 --views 100 --only batched --reps 3
--only batched | sequential | mesh runs one arm alone: under rocprofv3 --kernel-trace --stats that gives its kernels alone.
The scene: a sphere of radius 0.4 of the cube's side seen from cameras on a circle around it, analytic ray-sphere depth with a backdrop
behind the volume, so that every voxel in a frustum is updated (free space included): the expensive case.
GSR_LIB=path/to/libgsr_hip.so times another build."""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gsr = importlib.import_module("3dgs-native_amd")
W = H = 800
SIDE, RADIUS, DISTANCE, TAN = 2.0, 0.8, 4.0, 0.35


def camera(k, n):
    a = 2.0 * math.pi * k / n
    eye = np.array([DISTANCE * math.cos(a), DISTANCE * math.sin(a), 0.6 * math.sin(3 * a)])
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z], axis=1)
    M = np.eye(4)
    M[:3, :3], M[3, :3] = R, -eye @ R
    return {"world_to_camera": M.astype(np.float32), "tan_fovx": TAN, "tan_fovy": TAN, "width": W, "height": H}


def sphere_depth(cam, dev):
    """(H, W) view depth of the sphere at the origin, 2 * DISTANCE (a backdrop behind the volume) where the ray misses it."""
    c = torch.tensor(cam["world_to_camera"][3, :3], device=dev, dtype=torch.float64)           # the centre in camera space
    x = ((2 * torch.arange(W, device=dev, dtype=torch.float64) + 1) / W - 1) * TAN
    y = ((2 * torch.arange(H, device=dev, dtype=torch.float64) + 1) / H - 1) * TAN
    r = torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W), torch.ones((H, W), device=dev, dtype=torch.float64)], dim=-1)
    rr, rc = (r * r).sum(-1), r @ c
    disc = rc * rc - rr * (c @ c - RADIUS * RADIUS)
    z = (rc - disc.clamp_min(0).sqrt()) / rr
    return torch.where(disc > 0, z, torch.full_like(z, 2 * DISTANCE)).float().contiguous()


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--views", default="8,100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="all", choices=["all", "batched", "sequential", "mesh"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tsdf_bench needs the GPU"
    dev = torch.device("cuda", 0)
    L = gsr._lib.lib()
    color = torch.rand((H, W, 3), device=dev)
    result = {"lib": os.path.basename(gsr._lib.LIB_PATH), "image": f"{W}x{H}", "sizes": {}}
    for G in (int(g) for g in args.sizes.split(",")):
        s = SIDE / (G - 1)
        vol = gsr.tsdf.TSDFVolume((-0.5 * SIDE,) * 3, s, (G, G, G), device=dev)
        row = {"voxels": G ** 3, "integrate_ms": {}}
        for V in (int(v) for v in args.views.split(",")):
            cams = [camera(k, V) for k in range(V)]
            depths = [sphere_depth(c, dev) for c in cams]
            colors = [color] * V
            r = {"voxel_views": G ** 3 * V}
            if args.only in ("all", "batched"):
                vol.reset()
                r["batched"] = round(timed(lambda: vol.integrate_views(depths, cams, colors), args.reps), 3)
                r["batched_GB_moved"] = round(40e-9 * G ** 3 * -(-V // gsr._lib.TSDF_VIEWS_PER_LAUNCH), 2)
            if args.only in ("all", "sequential"):
                vol.reset()

                def one_by_one():
                    for z, c, col in zip(depths, cams, colors):
                        vol.integrate(z, c, color=col)
                r["sequential"] = round(timed(one_by_one, args.reps), 3)
                r["sequential_GB_moved"] = round(40e-9 * G ** 3 * V, 2)
            if "batched" in r and "sequential" in r:
                r["sequential_over_batched"] = round(r["sequential"] / r["batched"], 3)
            row["integrate_ms"][str(V)] = r
        if args.only in ("all", "mesh"):
            ax = torch.arange(G, device=dev, dtype=torch.float32) * s - 0.5 * SIDE
            vol.tsdf.copy_(((ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2).sqrt() - RADIUS) / vol.trunc)
            vol.tsdf.clamp_(-1.0, 1.0)
            vol.weight.fill_(1.0)
            vol.color.copy_(torch.rand_like(vol.color))
            v = vol._struct()
            stream = None
            count = lambda: gsr._lib.check(L.gsr_mesh_count(C.byref(v), 1.0, vol._ws.data_ptr(), vol._ws.numel(), vol._total.data_ptr(), stream))
            count()
            T = int(vol._total.item())
            vertices = torch.empty((T, 3, 3), device=dev)
            colors3 = torch.empty((T, 3, 3), device=dev)
            keys = torch.empty((T, 3), dtype=torch.int64, device=dev)
            emit = lambda: gsr._lib.check(L.gsr_mesh_emit(C.byref(v), 1.0, vol._ws.data_ptr(), vol._ws.numel(), T, vertices.data_ptr(),
                                                          colors3.data_ptr(), keys.data_ptr(), stream))
            row["mesh"] = {"cells": (G - 1) ** 3, "triangles": T, "count_ms": round(timed(count, args.reps), 3), "emit_ms": round(timed(emit, args.reps), 3),
                           "extract_mesh_ms": round(timed(lambda: vol.extract_mesh(1.0), args.reps), 3), "emit_MB_written": round(96e-6 * T, 1)}
        result["sizes"][str(G)] = row
        del vol
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
