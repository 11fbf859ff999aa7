#!/usr/bin/env python3
"""The bits of everything that ends in a fixed-order sum ("The fixed-order sum"), for comparing two builds of the library:
every entry point of exposure.hip, depth_corr.hip, dssim.hip, camera_bwd.hip and the four loss sums of train_ops.hip on seeded
inputs (tests/fixed_order_sum.py: its sizes and its inputs), every instantiation, and one JSON line of name -> sha256 of each
output buffer.
    GSR_LIB=ab/lib_parent.so python tools/fixed_sum_bits.py > parent.json;  python tools/fixed_sum_bits.py > new.json;  cmp parent.json new.json
The four sums of train_ops.hip end in one atomic per workgroup, so they are hashed only at sizes that launch one workgroup; their
gradient images at every size.  The camera gradient runs on seeded accumulators through gsr_backward_camera(_aa): the blend
backward's own accumulators come from float atomics and differ from run to run.
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/fixed_sum_bits.py --calls-only 20 --sizes 800x800
--calls-only N makes the same calls N times at the given sizes and hashes nothing: the kernels alone, for a kernel trace."""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
gsr = importlib.import_module("3dgs-native_amd")
import fixed_order_sum as FS                 # noqa: E402  (the model, its sizes and its inputs live with the tests)
from exposure_reference import case_sizes    # noqa: E402

OUT = {}
HASH = True


def put(name, *tensors):
    for k, t in enumerate(tensors):
        if HASH and t is not None:
            OUT[f"{name}[{k}]"] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def exposure_calls(W, H, q):
    X, tag, r, g = gsr.exposure, f"{W}x{H}", q["r"], q["g"]
    E = gpu((np.eye(4, 3) + 0.1).astype(np.float32).reshape(12))
    put(f"exposure_apply {tag}", X.apply_exposure(r, E))
    put(f"exposure_backward {tag}", *X.exposure_backward(r, E, g))
    put(f"exposure_backward sums only {tag}", X.exposure_backward(r, E, g, want_image_grad=False)[1])


def image_calls(W, H, q, one_workgroup_sums):
    """Every image-sized entry point at one size; q: fixed_order_sum inputs on the device."""
    loss = gsr.loss
    tag = f"{W}x{H}"
    m, r, t = q["m"], q["r"], q["t"]
    d_r, d_t, d_m = r[:, :, 0].contiguous(), t[:, :, 0].contiguous(), m.abs()
    exposure_calls(W, H, q)
    for mask in (None, d_m):
        for want_grad in (True, False):
            put(f"depth_corr mask={mask is not None} grad={want_grad} {tag}", *loss.depth_corr_loss_and_gradients(d_r, d_t, mask, 0.7, want_grad=want_grad))
    pw = loss.PixelWeights(m)
    put(f"weight_total {tag}", pw.total)
    for want_grad in (True, False):
        put(f"weighted_l1 grad={want_grad} {tag}", *loss.l1_loss_and_gradients(r, t, 0.2, want_grad=want_grad, weights=pw))
        for window in ("gaussian", "reference"):
            put(f"dssim {window} grad={want_grad} {tag}", *loss.l1_dssim_loss_and_gradients(r, t, 0.2, window=window, want_grad=want_grad))
            put(f"weighted_dssim {window} grad={want_grad} {tag}", *loss.l1_dssim_loss_and_gradients(r, t, 0.2, window=window, want_grad=want_grad, weights=pw))
    # train_ops.hip: the sums only where one workgroup adds them
    P = W * H
    s, grad = loss.l1_loss_and_gradients(r, t, 0.2)
    put(f"l1 {tag}", s if one_workgroup_sums and 3 * P <= 4 * 256 else None, grad)
    acc = torch.empty(1, dtype=torch.float32, device=r.device)
    L, _host = gsr._lib.lib(), gsr._host
    gsr._lib.check(L.gsr_ssim(_host.ptr(r), _host.ptr(t), _host.ptr(acc), W, H, _host.stream_ptr(r.device)))
    put(f"ssim {tag}", acc if one_workgroup_sums and W <= 16 and H <= 16 else None)
    gsr._lib.check(L.gsr_depth_loss(_host.ptr(d_r), _host.ptr(d_t), _host.ptr(d_m), _host.ptr(acc), W, H, _host.stream_ptr(r.device)))
    put(f"depth_loss {tag}", acc if one_workgroup_sums and P <= 256 else None)
    for name, fn in (("depth_loss_grad", loss.depth_loss_and_gradients), ("alpha_loss_grad", loss.alpha_loss_and_gradients)):
        for mask in (None, d_m):
            s, grad = fn(d_r, d_t, mask, 0.7)
            put(f"{name} mask={mask is not None} {tag}", s if one_workgroup_sums and P <= 256 else None, grad)


def exposure_adam():
    model = gsr.exposure.ExposureModel(2, torch.device("cuda", 0))
    grads = FS.spread_values((3, 12), 5, 1.0)
    for k in range(3):
        model.step(1, gpu(grads[k]), 0.01)
    put("exposure_adam", model.E, model.m, model.v)


def camera_calls(n, calls=1):
    """gsr_backward_camera and its antialiased twin on the geometry of a rendered frame and seeded accumulators."""
    _lib, _host = gsr._lib, gsr._host
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    W, H = 160, 120
    sc = gsr.scenes.synthetic_scene(n, 0.05, 0.6, 1)
    cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    kw = dict(background=np.zeros(3, np.float32), means3D=sc["means"], colors=None, opacity=sc["opacities"], scales=sc["scales"],
              rotations=sc["rotations"], scale_modifier=1.0, viewmatrix=cam["world_to_camera"], projmatrix=cam["full_proj_matrix"],
              tan_fovx=cam["tan_fovx"], tan_fovy=cam["tan_fovy"], image_height=H, image_width=W, sh=sc["shs"], degree=3,
              campos=cam["camera_center"], prefiltered=False, antialiasing=False, clamped=True)
    _, _, buf = gsr.render_gaussians(**kw)
    t = lambda a, shape: torch.as_tensor(np.ascontiguousarray(a, np.float32)).reshape(shape).to(dev)
    means, scales, rots = t(sc["means"], (n, 3)), t(sc["scales"], (n, 3)), t(sc["rotations"], (n, 4))
    op, shs = t(sc["opacities"], (n,)), t(sc["shs"], (n * 16, 3))
    scene = _lib.GsrScene(n, _host.ptr(means), _host.ptr(scales), _host.ptr(rots), _host.ptr(op), _host.ptr(shs), int(kw["degree"]),
                          float(kw["scale_modifier"]), 1)
    camera = _host.make_camera(kw["viewmatrix"], kw["projmatrix"], kw["campos"], kw["background"], kw["tan_fovx"], kw["tan_fovy"], W, H)
    geom = _lib.GsrGeom(_host.ptr(buf["radii"]), None, None, None, None, None, None, None, _host.ptr(buf["clamped_state"]), None, None)
    off, ws_bytes = int(L.gsr_backward_accumulators_offset(n)), int(L.gsr_backward_workspace_bytes(n, 0, W, H))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    ws[off:off + 64 * n] = gpu(FS.spread_values((n, 16), 11, 1.0) * np.float32(1e-3)).view(torch.uint8).reshape(-1)
    aa_scale = gpu(np.random.default_rng(12).uniform(0.5, 1.0, n).astype(np.float32))
    scratch = torch.empty(max(16, int(L.gsr_backward_camera_scratch_bytes(n))), dtype=torch.uint8, device=dev)
    for name, aa in (("camera classic", None), ("camera antialiased", aa_scale)):
        out = torch.full((36,), float("nan"), device=dev)
        for _ in range(calls):
            args = (C.byref(scene), C.byref(camera), C.byref(geom), _host.ptr(out), _host.ptr(ws), ws_bytes, _host.ptr(scratch), scratch.numel())
            _lib.check(L.gsr_backward_camera_aa(*args, _host.ptr(aa), _host.raw_stream(dev)) if aa is not None else
                       L.gsr_backward_camera(*args, _host.raw_stream(dev)))
        put(f"{name} n={n} visible={int((buf['radii'] > 0).sum())}", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls-only", type=int, default=0, metavar="N")
    ap.add_argument("--sizes", default="", help="image sizes WxH, separated by commas (default: the sizes of the bit tests)")
    ap.add_argument("--camera-n", default="300,70000", help="Gaussian counts of the camera calls (one workgroup of rows, several)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fixed_sum_bits needs the GPU"
    global HASH
    HASH = not args.calls_only
    torch.cuda.set_device(0)
    sizes = [tuple(int(x) for x in wh.split("x")) for wh in args.sizes.split(",")] if args.sizes else sorted(set(FS.flat_sizes() + FS.tile_sizes()))
    for W, H in sizes:
        q = {k: gpu(v) for k, v in FS.flat_inputs(W, H).items()}
        for _ in range(max(1, args.calls_only)):
            image_calls(W, H, q, one_workgroup_sums=not args.calls_only)
    if not args.sizes:   # exposure.hip's own edges (its 1024-block cap, its 16-float records): the exposure calls alone
        own = gsr._lib.EXPOSURE_BLOCK_PIXELS, gsr._lib.EXPOSURE_MAX_BLOCKS
        for W, H in (s for s in case_sizes(*own) if s not in sizes):
            exposure_calls(W, H, {k: gpu(v) for k, v in FS.flat_inputs(W, H, *own).items()})
    exposure_adam()
    for n in (int(x) for x in args.camera_n.split(",")):
        camera_calls(n, max(1, args.calls_only))
    torch.cuda.synchronize()
    print(json.dumps({"lib": os.path.basename(gsr._lib.LIB_PATH)} if args.calls_only else dict(sorted(OUT.items()))), flush=True)


if __name__ == "__main__":
    main()
