"""
The depth-distortion regulariser over the lists of a rendered frame (include/gsr_distortion.h) over the MI355X library: per pixel

    Dist(p) = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2 = A S,    A = sum w,  mu = sum w m / A,  S = sum w (m - mu)^2

with w the weights the frame was blended with and m the inverse view depth of each Gaussian -- the term 2DGS, GOF, PGSR and RaDe-GS
train with before they extract a mesh.

    image, depth, buffers = render_gaussians(...)                        # any rasterize_mode, with or without filter_3d
    dist, moments = render_distortion(buffers, H, W)                     # (H, W) and (H, W, 4) = (A, mu, S, 0), float32
    loss, g = loss.distortion_loss_and_gradients(dist, weight=lam)       # g = dL/d(dist), (H, W)
    grads = backward(..., dL_ddistortion=g, distortion_moments=moments)  # adds the term's gradient to every parameter

The forward gives the same bits every call.  Its gradient has no image to travel through (it depends on the pixel and the entry
together), so it is a stage of backward() between the blend half and the per-Gaussian half (backward.py).  A capacity-mode frame
is to be used only once rendered_count(buffers) has said that it did not overflow.  Everything is enqueued on the current stream;
nothing is read back.
"""
import ctypes as C

import torch

from . import _args, _host, _lib
from . import features as _features


def inv_depth_of(buffers, N, dev):
    """(N,) float32 view or tensor of 1 / view depth: column 9 of the forward's blend records while the frame's arrays are theirs
    and unwritten, else 1 / buffers['depths'] (0 where the depth is not positive, as the records have it)."""
    xy = buffers["points_xy_image"]
    tag = getattr(xy, "_gsr_records", None)
    if tag is not None:
        rec, stamps = tag
        given = {"means2D": xy, "conic_opacity": buffers["conic_opacity"], "rgb": buffers.get("colors")}
        if all(_host.unwritten(stamps[k], given.get(k)) for k in stamps) and rec.device == dev and tuple(rec.shape) == (N, 16):
            return rec[:, 9]
    d = buffers.get("depths")
    if not (_args.is_dev(d, torch.float32) and d.dim() == 1 and d.shape[0] == N):
        raise ValueError("buffers['depths'] must be a float32 device tensor of shape (N,) when the frame does not carry the forward's records")
    return torch.where(d > 0, 1.0 / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(d))


def frame_struct(fr, inv_depth, masks):
    """GsrDistortionFrame over the checked frame arrays of features._check_frame."""
    N, D, xy, co, pl, rg, nc = fr
    H, W = int(nc.shape[0]), int(nc.shape[1])
    return _lib.GsrDistortionFrame(W, H, N, D, xy.data_ptr(), int(xy.stride(0)), co.data_ptr(), int(co.stride(0)), _host.ptr(pl), _host.ptr(rg),
                                   _host.ptr(nc), _host.ptr(masks), inv_depth.data_ptr(), int(inv_depth.stride(0)))


def render_distortion(buffers, image_height, image_width, out=None, use_block_masks=True):
    """(dist, moments): (H, W) float32 Dist(p) and (H, W, 4) float32 (A, mu, S, 0), the running sums the backward needs.  `out`: a
    caller-owned (dist, moments) pair to write into (every element is written).  use_block_masks=False walks without the forward's
    block masks (the same bits either way)."""
    fr = _features._check_frame(buffers, image_height, image_width)
    H, W = int(image_height), int(image_width)
    if out is not None:
        if not (isinstance(out, (tuple, list)) and len(out) == 2):
            raise ValueError("out must be a (dist, moments) pair")
        _args.check_out(out[0], (H, W), "out[0]")
        _args.check_out(out[1], (H, W, 4), "out[1]")
        dist, moments = out
    N, D, xy = fr[0], fr[1], fr[2]
    dev = xy.device
    if out is None:
        dist = torch.empty((H, W), dtype=torch.float32, device=dev)
        moments = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    if N == 0:
        return dist.zero_(), moments.zero_()
    inv_depth = inv_depth_of(buffers, N, dev)
    _args.check_one_device(*fr[2:], dist, moments)
    masks = _features._masks_of(buffers, D, dev) if use_block_masks else None
    L = _lib.lib()
    frame = frame_struct(fr, inv_depth, masks)
    with _host.on_device(dev):
        _lib.check(L.gsr_distortion_forward(C.byref(frame), _host.ptr(dist), _host.ptr(moments), _host.raw_stream(dev)))
    _host.written_in_place(dist)
    _host.written_in_place(moments)
    return dist, moments


def check_gradient_pair(dL_ddistortion, distortion_moments):
    """backward()'s two keywords: both or neither."""
    if (dL_ddistortion is None) != (distortion_moments is None):
        raise ValueError("backward() needs dL_ddistortion and distortion_moments together: the moments are render_distortion()'s second result")
    return dL_ddistortion is not None
