#!/usr/bin/env python3
"""The bits of every float32 restatement under tests/ (features, distortion, rendered normals, plane depth), for comparing two
versions of the helper modules: each entry point on the CPU oracle's forward of features_reference.SCENES, as the oracle_case
helpers of the four test_*_reference.py files build them, and one JSON file of "entry point frame" -> sha256 of the output arrays
(dtype, shape and bytes).  No GPU.
    git archive HEAD~1 tests | tar -x -C /tmp/parent
    python tools/restatement_bits.py --tests /tmp/parent/tests --out parent.json
    python tools/restatement_bits.py --out new.json;  cmp parent.json new.json
--tests names the directory whose *_reference.py modules are digested; the oracle and the package are this tree's in both runs."""
import argparse
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tests", default=os.path.join(ROOT, "tests"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_walk_reference", "bits.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.abspath(args.tests))
    import distortion_reference as DR
    import features_reference as FR
    import normal_render_reference as NR
    import plane_depth_reference as PD
    from oracle import oracle
    oracle.lib()
    scenes, cameras = (importlib.import_module(f"3dgs-native_amd.{m}") for m in ("scenes", "cameras"))
    out = {}
    first = next(iter(FR.SCENES))
    for name in FR.SCENES:
        sc, cam, kw = FR.scene(scenes, cameras, name)
        H, W = kw["image_height"], kw["image_width"]
        buf = oracle.render_gaussians(**kw)[2]
        view = np.asarray(kw["viewmatrix"], f32)

        g = DR.draw_g(H, W)
        dist, mom = DR.forward_f32(buf, W, H)
        out[f"distortion.forward_f32 {name}"] = digest(dist, mom)
        out[f"distortion.backward_f32 {name}"] = digest(DR.backward_f32(buf, W, H, g, mom))
        if name == first:
            out[f"distortion.forward_f32 moments {name}"] = digest(*DR.forward_f32(buf, W, H, form="moments"))
            out[f"distortion.backward_f32 drop_suffix {name}"] = digest(DR.backward_f32(buf, W, H, g, mom, drop_suffix=True))

        n32 = NR.normals_f32(sc["scales"], sc["rotations"], sc["means"], view)[0]
        G = NR.draw_G(H, W)
        img = NR.render_f32(buf, W, H, n32)
        out[f"normal_render.render_f32 {name}"] = digest(img)
        out[f"normal_render.render_backward_f32 {name}"] = digest(*NR.render_backward_f32(buf, W, H, n32, G, img))
        if name == first:
            out[f"normal_render.render_backward_f32 drop_suffix {name}"] = digest(*NR.render_backward_f32(buf, W, H, n32, G, img, drop_suffix=True))

        sl = PD.slopes_f32(n32, PD.plane_scales(sc["scales"]), sc["means"], view, kw["tan_fovx"], kw["tan_fovy"], W, H)[0]
        fr = PD.frame_of_buffers(buf, W, H, PD.inv_depth_of_buffers(buf))
        gp = PD.draw_g(H, W)
        pimg, Tf = PD.render_f32(fr, sl)
        out[f"plane_depth.render_f32 {name}"] = digest(pimg, Tf)
        out[f"plane_depth.render_backward_f32 {name}"] = digest(*PD.render_backward_f32(fr, sl, gp, pimg))
        if name == first:
            out[f"plane_depth.render_backward_f32 drop_suffix {name}"] = digest(*PD.render_backward_f32(fr, sl, gp, pimg, drop_suffix=True))

        F, Gf = FR.draw(sc["means"].shape[0], 3, H, W)
        r = FR.render(buf, W, H, F, Gf)
        out[f"features.render out32 {name}"] = digest(r["out32"])
        out[f"features.render dF32 {name}"] = digest(r["dF32"])
        if name == "n900_faint_48x32":                  # the heaviest entry of the longest list, and the 8x4 block where it weighs most
            tile, xs, ys, idx, w, _ = max(r["tiles"], key=lambda t: len(t[3]))
            k = int(w.sum(0).argmax())
            blk = ((ys % 16) // 4) * 2 + (xs % 16) // 8
            at = int(np.asarray(buf["ranges"]).reshape(-1, 2)[tile, 0]) + k
            drops = (("entry", at), ("block", at, int(np.argmax([w[blk == b, k].sum() for b in range(8)]))))
            for drop, d in zip(drops, FR.render(buf, W, H, F, Gf, drops=drops)["dF32_dropped"]):
                assert not np.array_equal(d, r["dF32"]), drop
                out[f"features.render dF32_dropped {drop[0]} {name}"] = digest(d)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} digests -> {args.out}")


if __name__ == "__main__":
    main()
