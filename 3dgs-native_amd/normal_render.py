"""
The Gaussians' own normals as an image, and the pieces of the depth-normal consistency term (include/gsr_normal_render.h) over the
MI355X library -- the second geometric term 2DGS, GOF, PGSR and RaDe-GS train with before they extract a mesh.  A Gaussian's normal
is the direction of its shortest axis, turned to face the camera; the image blends them with the weights a frame was drawn with.

    image, depth, buffers = render_gaussians(...)                        # any rasterize_mode, with or without filter_3d
    n = gaussian_normals(scales, rotations, positions, camera)           # (N, 3) float32, camera space, facing the camera
    nimg = render_normals(n, buffers, H, W)                              # (H, W, 3): sum_k w_k(p) n[i_k]; bit for bit render_features(n)
    sums, gN, gD, gA = loss.normal_consistency_loss_and_gradients(nimg, depth, buffers["final_Ts"], camera, weight=lam)
    grads = backward(..., dL_ddepth_image=gD, dL_dalpha_image=gA, dL_dnormal_image=gN, gaussian_normals=n, normal_image=nimg)

The image's gradient reaches the rotations through the normals AND the opacities, positions and shapes through the weights: it
depends on the pixel and the entry together, so it is a stage of backward() between the blend half and the per-Gaussian half
(backward.py), like the distortion term.  `camera`: a dict with world_to_camera (4 x 4, row-vector convention).  The forward gives
the same bits every call.  A capacity-mode frame is to be used only once rendered_count(buffers) has said that it did not overflow.
Everything is enqueued on the current stream; nothing is read back.
"""
import ctypes as C

import numpy as np
import torch

from . import _args, _frame, _host, _lib


def view_floats(viewmatrix, who):
    """The 16 host floats of a view matrix (row-vector convention), checked: (ctypes array, numpy array)."""
    if isinstance(viewmatrix, dict):
        if "world_to_camera" not in viewmatrix:
            raise ValueError(f"{who}: camera must be a dict with world_to_camera, or a 4 x 4 view matrix")
        viewmatrix = viewmatrix["world_to_camera"]
    if isinstance(viewmatrix, torch.Tensor):
        viewmatrix = viewmatrix.detach().cpu().numpy()
    try:
        v = np.asarray(viewmatrix, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: the view matrix must be a 4 x 4 array of numbers") from None
    if v.size != 16 or not np.isfinite(v).all():
        raise ValueError(f"{who}: the view matrix must be a finite 4 x 4 matrix, not shape {v.shape}")
    v = np.ascontiguousarray(v.reshape(16).astype(np.float32))
    return v.ctypes.data_as(C.POINTER(C.c_float)), v


def _check_gaussians(scales, rotations, means, who):
    """Three float32 device tensors (N, 3), (N, 4), (N, 3); returns N."""
    for name, t, width in (("scales", scales, 3), ("rotations", rotations, 4), ("means", means, 3)):
        if not (_args.is_dev(t, torch.float32) and t.dim() == 2 and t.shape[1] == width):
            raise ValueError(f"{who}: {name} must be a float32 device tensor of shape (N, {width})")
    N = int(scales.shape[0])
    if int(rotations.shape[0]) != N or int(means.shape[0]) != N:
        raise ValueError(f"{who}: scales, rotations and means disagree on the number of Gaussians")
    return N


def gaussian_normals(scales, rotations, means, camera, out=None):
    """(N, 3) float32: the unit normal of every Gaussian in camera space -- the column of its rotation matrix (csrc/sigma3d.h's, the
    quaternion as stored) that belongs to its smallest scale (ties: the lower index), turned so that it faces the camera; (0, 0, 0)
    for a zero quaternion.  `camera`: a dict with world_to_camera, or the 4 x 4 view matrix itself.  `out`: a caller-owned (N, 3)
    tensor to write into."""
    who = "gaussian_normals"
    N = _check_gaussians(scales, rotations, means, who)
    vp, keep = view_floats(camera, who)
    if out is not None:
        _args.check_out(out, (N, 3), "out")
    _args.check_one_device(scales, rotations, means, out)
    dev = scales.device
    if out is None:
        out = torch.empty((N, 3), dtype=torch.float32, device=dev)
    if N == 0:
        return out
    L = _lib.lib()
    sc, rot, mu = (_host.to_dev(t, torch.float32, dev) for t in (scales, rotations, means))
    with _host.on_device(dev):
        _lib.check(L.gsr_gaussian_normals(N, _host.ptr(sc), _host.ptr(rot), _host.ptr(mu), vp, _host.ptr(out), _host.raw_stream(dev)))
    _host.written_in_place(out)
    return out


def gaussian_normals_backward(dL_dnormals, scales, rotations, means, camera, dL_drot=None):
    """ADDS to `dL_drot` (N, 4) (None: a fresh zero tensor) the derivative of gaussian_normals() with respect to the stored
    quaternions, the choice of axis and the facing held constant, and returns it.  Nothing flows to scales, means or the camera."""
    who = "gaussian_normals_backward"
    N = _check_gaussians(scales, rotations, means, who)
    vp, keep = view_floats(camera, who)
    if not (_args.is_dev(dL_dnormals, torch.float32) and tuple(dL_dnormals.shape) == (N, 3) and dL_dnormals.is_contiguous()):
        raise ValueError(f"{who}: dL_dnormals must be a contiguous float32 device tensor of shape (N, 3)")
    if dL_drot is not None:
        _args.check_out(dL_drot, (N, 4), "dL_drot")
    _args.check_one_device(scales, rotations, means, dL_dnormals, dL_drot)
    dev = scales.device
    if dL_drot is None:
        dL_drot = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    if N == 0:
        return dL_drot
    L = _lib.lib()
    sc, rot, mu, g = (_host.to_dev(t, torch.float32, dev) for t in (scales, rotations, means, dL_dnormals))
    with _host.on_device(dev):
        _lib.check(L.gsr_gaussian_normals_backward(N, _host.ptr(sc), _host.ptr(rot), _host.ptr(mu), vp, _host.ptr(g), _host.ptr(dL_drot),
                                                   _host.raw_stream(dev)))
    _host.written_in_place(dL_drot)
    return dL_drot


def render_normals(normals, buffers, image_height, image_width, out=None, use_block_masks=True):
    """(H, W, 3) float32: out[y, x] = sum over the pixel's contributing list entries of w_k * normals[i_k], front to back, one fused
    multiply-add per term: bit for bit features.render_features(normals, ...).  No background is added, and the image is not
    normalised (its length is at most the coverage 1 - final_Ts).  `out`: a caller-owned tensor to write into (every element is
    written).  use_block_masks=False walks without the forward's block masks (the same bits either way)."""
    fr = _frame.Frame.from_buffers(buffers, image_height, image_width, use_block_masks)
    if not (_args.is_dev(normals, torch.float32) and tuple(normals.shape) == (fr.N, 3) and normals.is_contiguous()):
        raise ValueError("normals must be a contiguous float32 device tensor of shape (N, 3) with N the frame's number of Gaussians")
    out, = fr.outputs(out, [(fr.H, fr.W, 3)], (normals,))
    if fr.N == 0:
        return out.zero_()
    n = _host.to_dev(normals, torch.float32, fr.device)
    fr.launch("gsr_normal_render_forward", _host.ptr(n), _host.ptr(out), written=(out,))
    return out


STAGE_KEYWORDS = {"dL_dnormal_image": None, "gaussian_normals": None, "normal_image": None, "normal_param_grad": True}   # name: default


def stage_keywords(kw):
    """backward()'s keywords of this stage out of its catch-all dict, in STAGE_KEYWORDS' order with their defaults; a name that is
    not one of them is refused as Python refuses an unknown keyword."""
    for name in kw:
        if name not in STAGE_KEYWORDS:
            raise TypeError(f"backward() got an unexpected keyword argument '{name}'")
    return tuple(kw.get(name, default) for name, default in STAGE_KEYWORDS.items())


def check_gradient_triple(dL_dnormal_image, gaussian_normals, normal_image):
    """backward()'s three keywords: all or none."""
    given = [x is not None for x in (dL_dnormal_image, gaussian_normals, normal_image)]
    if any(given) and not all(given):
        raise ValueError("backward() needs dL_dnormal_image, gaussian_normals and normal_image together: the normals are "
                         "gaussian_normals()'s result, the image render_normals()'s")
    return all(given)
