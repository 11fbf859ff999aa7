#!/usr/bin/env python3
"""The bits of every forward that replays a finished frame's tile lists, through the PUBLIC Python API only (so the same file runs
against another checkout's package): for comparing two versions of the host layer over one library.  One JSON line of
name -> sha256 of each output.
    GSR_LIB=$PWD/3dgs-native_amd/libgsr_hip.so python tools/frame_stage_bits.py --package-root ab/parent > parent.json
    GSR_LIB=$PWD/3dgs-native_amd/libgsr_hip.so python tools/frame_stage_bits.py > new.json;  cmp parent.json new.json
`--package-root DIR`: the directory that holds the package directory (default: this checkout).  Two seeded frames of 2000 synthetic
Gaussians (scenes.synthetic_scene(2000, 0.05, 0.6, 2), the first NeRF-synthetic lego pose): 64 x 48 and 50 x 37 (partial tiles).
On each: render_features at C = 1, 3 and 33, render_distortion, gaussian_normals, render_normals, plane_slopes, render_plane_depth
and render_median_depth, each with use_block_masks on and off, on the forward's own buffers and on buffers whose points_xy_image
and conic_opacity are clones (no records behind them: 1 / depth then comes from buffers["depths"], and the block masks' stamps do
not hold).  All of these give the same bits every call; the backwards end in float atomics and are left to the tests."""
import argparse
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    gsr = importlib.import_module("3dgs-native_amd")
    feat, dist, nr, md, pd = gsr.features, gsr.distortion, gsr.normal_render, gsr.median_depth, gsr.plane_depth
    assert torch.cuda.is_available(), "frame_stage_bits needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)
    sc = gsr.scenes.synthetic_scene(2000, 0.05, 0.6, 2)
    N = sc["means"].shape[0]
    means, scales, rotations = t(sc["means"]), t(sc["scales"]), t(sc["rotations"])
    out = {}

    def put(name, *tensors):
        for k, x in enumerate(tensors):
            out[f"{name}[{k}]"] = hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    for W, H in ((64, 48), (50, 37)):
        cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
        image, depth, own = gsr.render_gaussians(
            background=np.zeros(3, np.float32), means3D=means, opacity=t(sc["opacities"]), scales=scales, rotations=rotations,
            viewmatrix=cam["world_to_camera"], projmatrix=cam["full_proj_matrix"], tan_fovx=cam["tan_fovx"], tan_fovy=cam["tan_fovy"],
            image_height=H, image_width=W, sh=t(sc["shs"]), degree=3, campos=cam["camera_center"])
        put(f"{W}x{H} render_gaussians", image, depth, own["point_list"], own["ranges"], own["n_contrib"])
        normals = nr.gaussian_normals(scales, rotations, means, cam)
        slopes = pd.plane_slopes(normals, scales, means, cam)
        put(f"{W}x{H} gaussian_normals", normals)
        put(f"{W}x{H} plane_slopes", slopes)
        clones = dict(own, points_xy_image=own["points_xy_image"].clone(), conic_opacity=own["conic_opacity"].clone())
        rng = np.random.default_rng(11)
        F = {C: t(rng.uniform(-1, 1, (N, C))) for C in (1, 3, 33)}
        for tag, buf in (("own", own), ("clones", clones)):
            for masks in (True, False):
                name = f"{W}x{H} {tag} masks={masks}"
                for C, f in F.items():
                    put(f"{name} render_features C={C}", feat.render_features(f, buf, H, W, use_block_masks=masks))
                put(f"{name} render_distortion", *dist.render_distortion(buf, H, W, use_block_masks=masks))
                put(f"{name} render_normals", nr.render_normals(normals, buf, H, W, use_block_masks=masks))
                put(f"{name} render_plane_depth", pd.render_plane_depth(slopes, buf, H, W, use_block_masks=masks))
                put(f"{name} render_median_depth", *md.render_median_depth(buf, H, W, use_block_masks=masks))
    torch.cuda.synchronize()
    print(json.dumps(dict(sorted(out.items()))), flush=True)


if __name__ == "__main__":
    main()
