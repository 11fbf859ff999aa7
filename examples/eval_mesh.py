"""
Geometric error of a triangle mesh against a ground-truth surface: accuracy, completeness, Chamfer distance and F-score between
points sampled on both by area (include/gsr_mesh_eval.h, mesh_eval.py) -- the numbers 2DGS, GOF, PGSR and RaDe-GS report, on the
MI355X.

    python examples/eval_mesh.py --mesh mesh.ply --gt truth.ply --samples 1000000 --thresholds 0.01 0.02 --json eval.json
    python examples/eval_mesh.py --mesh mesh.ply --gt scan_points.ply --gt-points --max-dist 0.2 --crop -1 -1 -1 1 1 1
    python examples/eval_mesh.py --demo torus --resolution 128 --views 32

Both files are binary little-endian PLY in ONE frame: nothing here aligns a mesh to its ground truth.  --density D (samples per
unit area, on both meshes) or --samples S (about S on each; the default, 1 000 000).  --max-dist X sets points without a neighbour
within X aside as outliers (the DTU convention); --crop keeps the points inside a box.

--demo torus needs no file: it samples a parametric torus, starts Gaussians at the samples (point_cloud.gaussians_from_points),
renders them from orbiting cameras, fuses the depth into a TSDF volume of --resolution voxels per side, extracts the mesh and
evaluates it against the torus: the bias of render -> TSDF -> mesh, reported in voxels.  --depth-mode median fuses the median depth
(median_depth.py: the Gaussian at which the transmittance falls through one half) instead of the expected inverse depth;
--depth-mode plane fuses the ray-plane intersection depth (plane_depth.py), --depth-mode plane-median that depth under the median rule,
and --demo-flat RATIO makes the demo's Gaussians discs on the torus, which both need: an isotropic Gaussian has no plane and keeps its
centre depth.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def evaluate_mesh(gsr, verts, faces, gt_verts, gt_faces=None, density=None, samples=None, seed=0, log=print, **kw):
    """Sample the mesh (and the ground truth, unless gt_faces is None: then gt_verts are its points) and evaluate.  What this file
    and extract_mesh.py --gt both call.  Returns mesh_eval.evaluate's dict with the sampling figures."""
    import torch
    me = gsr.mesh_eval
    if density is None and samples is None:
        samples = 1_000_000
    pred, _ = me.sample_mesh(me.soup(verts, faces), density=density, samples=samples, seed=seed)
    if gt_faces is None:
        gt = torch.as_tensor(np.ascontiguousarray(gt_verts, np.float32))
    else:
        gt, _ = me.sample_mesh(me.soup(gt_verts, gt_faces), density=density, samples=samples, seed=seed + 1)
    m = me.evaluate(pred, gt, **kw)
    m.update(density=density, samples=samples, seed=seed)
    log(f"eval: accuracy {m['accuracy']:.6g}, completeness {m['completeness']:.6g}, chamfer {m['chamfer']:.6g}; F-score "
        + ", ".join(f"{f:.4f} at {t:g}" for t, f in zip(m["thresholds"], m["fscore"])) + f"; {m['n_pred']} against {m['n_gt']} points")
    return m


def torus_mesh(R, r, nu, nv):
    """(verts (nu nv, 3) float32, faces (2 nu nv, 3) int32) of the torus about the z axis: major radius R, tube radius r."""
    u, v = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    ring = R + r * np.cos(v)
    verts = np.stack([ring * np.cos(u), ring * np.sin(u), r * np.sin(v)], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)]).astype(np.int32)
    return verts, faces


def orbit_cameras(gsr, views, distance, size, angle_x):
    """`views` cameras on a spiral about the origin, elevations from -50 to +50 degrees, looking at it (Blender axes, as nerf_camera takes)."""
    cams = []
    for k in range(views):
        az = 2 * np.pi * k * 0.381966                          # golden-angle steps: no two views share a meridian
        el = np.radians(-50 + 100 * (k + 0.5) / views)
        eye = distance * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        z = eye / np.linalg.norm(eye)                          # the camera looks along -z
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        c2w = np.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, np.cross(z, x), z, eye
        cams.append(gsr.cameras.nerf_camera(c2w, size, size, angle_x))
    return cams


def flat_discs(P, R, ratio):
    """The demo's isotropic Gaussians turned into discs on the torus: the shortest axis (z of the local frame) along the torus's
    analytic normal at the Gaussian's centre, the in-plane scales the kNN scale the Gaussian had, the thickness `ratio` times it."""
    import torch
    p = P["positions"]
    rho = torch.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2).clamp_min(1e-12)
    ring = torch.stack([R * p[:, 0] / rho, R * p[:, 1] / rho, torch.zeros_like(rho)], 1)          # the nearest point of the centre circle
    n = torch.nn.functional.normalize(p - ring, dim=1)
    # the shortest rotation that takes e_z to n: q = (e_z x n, 1 + e_z . n), normalised, as (x, y, z, w)
    q = torch.stack([-n[:, 1], n[:, 0], torch.zeros_like(rho), 1.0 + n[:, 2]], 1)
    q = torch.where((q.norm(dim=1, keepdim=True) > 1e-6), q, torch.tensor([1.0, 0.0, 0.0, 0.0], device=p.device).expand_as(q))
    P["rotations"] = torch.nn.functional.normalize(q, dim=1).contiguous()
    s = P["scales"].clone()
    s[:, 2] = float(ratio) * s[:, :2].min(dim=1).values
    P["scales"] = s.contiguous()
    return P


def demo_torus(gsr, resolution, views, points, image_size, seed=0, log=print, depth_mode="expected", flat=None):
    import torch
    me = gsr.mesh_eval
    R, r, half = 0.6, 0.25, 1.0
    verts, faces = torus_mesh(R, r, 256, 128)
    start, _ = me.sample_mesh(me.soup(verts, faces), samples=points, seed=seed)
    P = gsr.point_cloud.gaussians_from_points(start.cpu().numpy(), opacity=0.9, device="cuda")
    if flat is not None:
        P = flat_discs(P, R, flat)
    plane = {"plane": True, "plane-median": "median"}.get(depth_mode, False)       # tsdf.fuse_views' keyword of its own
    cams = orbit_cameras(gsr, views, 3.0, image_size, 0.6911112070083618)
    bg = np.zeros(3, np.float32)
    mverts, mfaces, _, info = gsr.tsdf.fuse_views(lambda c: gsr.render_view(P, c, bg), cams, resolution=resolution, centre=(0.0, 0.0, 0.0), half_side=half,
                                                  depth_mode="expected" if plane else depth_mode, plane_depth=plane, params=P if plane else None)
    torch.cuda.synchronize()
    if info["triangles"] < 1:
        raise SystemExit("--demo torus: the extraction gave no triangle (more --views or a lower --resolution)")
    h = info["voxel_size"]
    m = evaluate_mesh(gsr, mverts, mfaces, verts, faces, samples=200_000, seed=seed + 1, thresholds=(h, 2 * h, 4 * h), log=log)
    m.update(demo="torus", depth_mode=depth_mode, resolution=info["resolution"], views=views, voxel_size=h, triangles=info["triangles"], vertices=info["vertices"],
             gaussians=int(start.shape[0]), image_size=image_size, flat=flat, accuracy_voxels=m["accuracy"] / h, completeness_voxels=m["completeness"] / h)
    if plane:
        m["plane_depth"] = info["plane_depth"]                  # fuse_views' own record of the keyword: True, or "median"
    log(f"demo torus ({depth_mode} depth): {m['gaussians']} Gaussians, {views} views of {image_size}^2 into {m['resolution']}^3 voxels of {h:.5f}: accuracy "
        f"{m['accuracy_voxels']:.3f} voxels, completeness {m['completeness_voxels']:.3f} voxels, {m['triangles']} triangles")
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", default=None, help="the mesh to judge (point_cloud.save_mesh_ply's format)")
    ap.add_argument("--gt", default=None, help="the ground truth: a mesh, or with --gt-points a point cloud")
    ap.add_argument("--gt-points", action="store_true", help="--gt holds points (its vertices), not a surface to sample")
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--density", type=float, default=None, metavar="D", help="samples per unit area")
    how.add_argument("--samples", type=int, default=None, metavar="S", help="about S samples per mesh (default 1 000 000)")
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.01, 0.02, 0.05], metavar="TAU")
    ap.add_argument("--max-dist", type=float, default=None, metavar="X")
    ap.add_argument("--crop", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None, metavar="OUT", help="write the result as JSON")
    ap.add_argument("--demo", choices=["torus"], default=None)
    ap.add_argument("--resolution", type=int, default=128, metavar="R", help="--demo: voxels per side")
    ap.add_argument("--views", type=int, default=32, metavar="V", help="--demo: orbit views")
    ap.add_argument("--demo-points", type=int, default=100_000, metavar="N", help="--demo: Gaussians on the torus")
    ap.add_argument("--demo-image", type=int, default=256, metavar="PX", help="--demo: image side")
    ap.add_argument("--depth-mode", choices=["expected", "median", "plane", "plane-median"], default="expected", help="--demo: the depth the "
                    "volume is fused from (plane: the ray-plane intersection depth under the expected blend, plane-median: under the median "
                    "rule, plane_depth.py)")
    ap.add_argument("--demo-flat", type=float, default=None, metavar="RATIO", help="--demo: turn the Gaussians into discs on the torus: normal = "
                    "the torus's analytic normal, in-plane scales = the kNN scale, thickness = RATIO times it.  Without it the demo's "
                    "isotropic Gaussians all fall back to their centre depth and --depth-mode plane / plane-median measure nothing")
    args = ap.parse_args()
    if args.demo is None and (args.mesh is None or args.gt is None):
        ap.error("--mesh and --gt are required (or --demo torus)")
    if args.demo is not None and not (2 <= args.resolution <= 2048 and args.views >= 1 and args.demo_points >= 4 and args.demo_image >= 8):
        ap.error("--demo: --resolution must be in 2 .. 2048, --views >= 1, --demo-points >= 4, --demo-image >= 8")
    if args.demo_flat is not None and not 0.0 < args.demo_flat <= 1.0:
        ap.error("--demo-flat must lie in (0, 1]")
    gsr = importlib.import_module("3dgs-native_amd")
    if args.demo:
        m = demo_torus(gsr, args.resolution, args.views, args.demo_points, args.demo_image, seed=args.seed, depth_mode=args.depth_mode, flat=args.demo_flat)
    else:
        try:
            verts, faces, _ = gsr.point_cloud.load_mesh_ply(args.mesh)
            if args.gt_points:
                gt_verts, gt_faces = gsr.point_cloud.load_points(args.gt)[0], None
            else:
                gt_verts, gt_faces, _ = gsr.point_cloud.load_mesh_ply(args.gt)
        except (OSError, ValueError) as e:
            raise SystemExit(f"eval_mesh: {e}")
        bounds = None if args.crop is None else (args.crop[:3], args.crop[3:])
        m = evaluate_mesh(gsr, verts, faces, gt_verts, gt_faces, density=args.density, samples=args.samples, seed=args.seed,
                          thresholds=args.thresholds, max_dist=args.max_dist, bounds=bounds)
        m.update(mesh=args.mesh, gt=args.gt, gt_points=bool(args.gt_points))
    print(json.dumps(m))
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(m) + "\n")


if __name__ == "__main__":
    main()
