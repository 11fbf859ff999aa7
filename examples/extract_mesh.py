"""
Triangle mesh of a trained model: render depth and colour from a dataset's cameras, fuse them into a truncated signed distance
volume and extract the zero level set by marching tetrahedra (include/gsr_tsdf.h, tsdf.py) -- the step 2DGS, GOF, PGSR and RaDe-GS
end with, on the MI355X and without Open3D.

    python examples/extract_mesh.py --model out/point_cloud/iteration_7000/point_cloud.ply --dataset data/lego --resolution 512 --out mesh.ply

The cube is centred on the cameras' common look-at point with half of their extent as its half side (tsdf.scene_bounds) unless
--center / --half-side name it.  --voxel-size S or --resolution R (voxels per side; default 256) set the grid, --trunc the
truncation distance (default 4 voxels), --depth-max drops far depths, --min-weight K keeps only cells all of whose corners were
observed with weight K.  Extraction is offline: it reads the triangle count back once, and welds on the host.
--depth-mode median fuses the median depth (median_depth.py: the depth of the Gaussian at which the transmittance falls through one
half, what the surface methods fuse bounded scenes from) instead of the expected inverse depth over the coverage; --depth-mode plane
fuses the ray-plane intersection depth (plane_depth.py: a flat Gaussian contributes the depth at which the pixel's ray meets its plane);
--depth-mode plane-median fuses that depth under the median rule (the plane of the one Gaussian at which the transmittance falls
through one half: what RaDe-GS and GOF fuse).
--gt G.ply evaluates the mesh right away against a ground truth in the same frame (accuracy, completeness, F-score: eval_mesh.py).
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def load_cameras(gsr, path, max_views, split="train"):
    """The dataset's cameras (NeRF-synthetic transforms_<split>.json); the image size is the first frame's."""
    from PIL import Image
    angle, frames = gsr.cameras.nerf_frames(path, max_views or None, split)
    with Image.open(frames[0][1]) as im:
        W, H = im.size
    return [gsr.cameras.nerf_camera(pose, W, H, angle) for _, _, _, pose in frames]


def mesh_from_model(gsr, P, cams, out, bg=None, mode_kw=None, log=print, **fuse):
    """Render `cams` from the parameter dict P (positions, scales, rotations, opacities, shs), fuse, extract, weld and write `out`.
    What examples/extract_mesh.py and train.py --mesh-out both call.  Returns fuse_views' info with the wall time."""
    import torch
    bg = np.zeros(3, np.float32) if bg is None else bg

    def render(c):
        return gsr.render_view(P, c, bg, **(mode_kw or {}))
    t0 = time.perf_counter()
    if fuse.get("depth_mode") in ("plane", "plane-median"):    # the depth model, not a blending rule: tsdf.fuse_views' keyword of its own
        fuse = dict(fuse, depth_mode="expected", plane_depth=True if fuse["depth_mode"] == "plane" else "median", params=P)
    verts, faces, cols, info = gsr.tsdf.fuse_views(render, cams, **fuse)
    torch.cuda.synchronize()
    info["fuse_extract_weld_s"] = round(time.perf_counter() - t0, 3)
    gsr.point_cloud.save_mesh_ply(out, verts, faces, cols)
    info["out"] = str(out)
    log(f"mesh: {info['triangles']} triangles, {info['vertices']} vertices from {info['views']} views into {info['resolution']}^3 voxels of "
        f"{info['voxel_size']:.5f} in {info['fuse_extract_weld_s']} s -> {out}")
    return info


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True, help="a checkpoint written by train.py (point_cloud.save_ply)")
    ap.add_argument("--dataset", required=True, help="NeRF-synthetic directory: its training cameras are the views")
    ap.add_argument("--views", type=int, default=0, metavar="N", help="use the first N cameras (0 = all)")
    grid = ap.add_mutually_exclusive_group()
    grid.add_argument("--voxel-size", type=float, default=None, metavar="S")
    grid.add_argument("--resolution", type=int, default=None, metavar="R", help="voxels per side (default 256)")
    ap.add_argument("--trunc", type=float, default=None, metavar="T", help="truncation distance (default 4 voxels)")
    ap.add_argument("--depth-max", type=float, default=float("inf"), metavar="D")
    ap.add_argument("--min-weight", type=float, default=1.0, metavar="K")
    ap.add_argument("--center", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    ap.add_argument("--half-side", type=float, default=None, metavar="E")
    ap.add_argument("--depth-mode", choices=["expected", "median", "plane", "plane-median"], default="expected",
                    help="the depth the volume is fused from")
    ap.add_argument("--out", default="mesh.ply")
    ap.add_argument("--record", default=None, metavar="FILE", help="write the run's figures (resolution, triangles, seconds) as one JSON line")
    ap.add_argument("--gt", default=None, metavar="G.ply", help="evaluate the mesh against this ground truth in the same frame (examples/eval_mesh.py)")
    ap.add_argument("--gt-points", action="store_true", help="--gt holds points, not a surface to sample")
    ap.add_argument("--eval-samples", type=int, default=1_000_000, metavar="S", help="--gt: about S samples per mesh")
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.01, 0.02, 0.05], metavar="TAU", help="--gt: F-score thresholds")
    ap.add_argument("--max-dist", type=float, default=None, metavar="X", help="--gt: points without a neighbour within X are outliers")
    args = ap.parse_args()
    if args.voxel_size is not None and not args.voxel_size > 0.0:
        raise SystemExit("--voxel-size must be positive")
    if args.resolution is not None and not 2 <= args.resolution <= 2048:
        raise SystemExit("--resolution must be in 2 .. 2048")
    import torch
    gsr = importlib.import_module("3dgs-native_amd")
    dev = torch.device("cuda", 0)
    ply = gsr.point_cloud.load_ply(args.model)
    P = {"positions": torch.as_tensor(ply["positions"]).to(dev), "scales": torch.as_tensor(ply["scales"]).to(dev),
         "rotations": torch.as_tensor(ply["rotations"]).to(dev), "opacities": torch.as_tensor(ply["opacities"]).reshape(-1, 1).to(dev),
         "shs": torch.as_tensor(ply["shs"]).to(dev)}
    cams = load_cameras(gsr, args.dataset, args.views)
    info = mesh_from_model(gsr, P, cams, args.out, voxel_size=args.voxel_size, resolution=args.resolution or 256, centre=args.center,
                           half_side=args.half_side, trunc=args.trunc, depth_max=args.depth_max, min_weight=args.min_weight, depth_mode=args.depth_mode)
    if args.gt:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from eval_mesh import evaluate_mesh
        verts, faces, _ = gsr.point_cloud.load_mesh_ply(args.out)
        if args.gt_points:
            gt_verts, gt_faces = gsr.point_cloud.load_points(args.gt)[0], None
        else:
            gt_verts, gt_faces, _ = gsr.point_cloud.load_mesh_ply(args.gt)
        info["eval"] = evaluate_mesh(gsr, verts, faces, gt_verts, gt_faces, samples=args.eval_samples, thresholds=args.thresholds, max_dist=args.max_dist)
        info["eval"]["gt"] = args.gt
    if args.record:
        with open(args.record, "w") as f:
            f.write(json.dumps(info) + "\n")


if __name__ == "__main__":
    main()
