"""
The 3D smoothing filter of Mip-Splatting (include/gsr_filter3d.h) over the MI355X library: a lower bound on every Gaussian's
world-space size, set by what the training views could resolve.

    f = compute_filter_3d(means3D, cameras)                    # (N,) float32: sqrt(0.2) / nu_i, nu_i = max over seeing views of focal / z
    s1, o1 = apply_filter_3d(scales, opacity, f)               # s' = sqrt(s^2 + f^2), opacity' = opacity * prod |s| / s'
    filter_3d_backward(scales, opacity, f, dL_ds1, dL_do1)     # the transpose, in place by default

render_gaussians(..., filter_3d=f) renders the filtered scene and backward(..., filter_3d=f) returns gradients with respect to the
RAW scales and opacity; both are exactly the substitution above around the unchanged kernels.  `f` is a pure function of the
positions and the cameras (max and min do not depend on order): every rank of a data-parallel run computes the same bits, so no
collective is needed.  It is recomputed when the point set changes, not every iteration (examples/train.py --filter-3d).
"""
import numpy as np
import torch

from . import _args, _host, _lib

_VIEW_DTYPE = np.dtype([("view", "<f4", (16,)), ("focal", "<f4"), ("W", "<i4"), ("H", "<i4"), ("pad", "<i4")])   # GsrFilterView, 80 bytes
_views = {}


def _view_record(cam):
    """(16 view floats, focal_x, W, H) of one camera: a trainer's camera dict (cameras.nerf_camera: `world_to_camera` is what it
    renders with), a packed _lib.GsrCamera, or a (viewmatrix, focal_x, W, H) tuple.  The focal length of a dict is focal_x as
    _host.make_camera forms it: W / (2 tan_fovx) in float64, rounded once by the float32 store."""
    if isinstance(cam, dict):
        return _host.host_f32(cam["world_to_camera"], 16), cam["width"] / (2.0 * float(cam["tan_fovx"])), cam["width"], cam["height"]
    if isinstance(cam, _lib.GsrCamera):
        return np.asarray(cam.view[:], np.float32), cam.focal_x, cam.W, cam.H
    view, focal, W, H = cam
    return _host.host_f32(view, 16), float(focal), W, H


def pack_views(cameras, dev):
    """The camera set as V GsrFilterView records on the device.  Packed once per camera set: the tensor is kept under the bytes
    of the records, so a trainer that comes back with the same (or equal) cameras uploads nothing."""
    rec = np.zeros(len(cameras), _VIEW_DTYPE)
    for k, cam in enumerate(cameras):
        rec["view"][k], rec["focal"][k], rec["W"][k], rec["H"][k] = _view_record(cam)
    key = (rec.tobytes(), dev.index)
    t = _views.get(key)
    if t is None:
        if len(_views) >= 64:
            _views.clear()
        t = _views[key] = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev) if len(rec) else torch.empty(0, dtype=torch.uint8, device=dev)
    return t, len(rec)


def compute_filter_3d(means3D, cameras, variance=_lib.FILTER3D_VARIANCE, out=None):
    """filter_3d (N,) float32 on the device, from all `cameras` (gsr_filter3d_from_views).  No camera, or no Gaussian seen by any:
    zeros, the pass-through.  `out`: a caller-owned (N,) float32 device tensor to write into."""
    variance = _args.positive(variance, "variance")
    L = _lib.lib()
    dev = _host.device_of(means3D, out)
    means = _host.to_dev(means3D, torch.float32, dev, (-1, 3))
    N = means.shape[0]
    if out is None:
        out = torch.empty((N,), dtype=torch.float32, device=dev)
    else:
        check_filter_3d(out, means)
    views, V = pack_views(list(cameras), dev)
    stream = _host.raw_stream(dev)
    with _host.on_device(dev):
        ws = _host.workspace("filter3d", L.gsr_filter3d_workspace_bytes(N), dev, stream)
        _lib.check(L.gsr_filter3d_from_views(N, _host.ptr(means), V, _host.ptr(views), variance, _host.ptr(out), _host.ptr(ws), ws.numel(), stream))
    _host.written_in_place(out)
    return out


def check_filter_3d(filter_3d, means3D):
    """The `filter_3d` keyword of render_gaussians() and backward(): refused before the library is touched unless it is a packed,
    16-byte aligned float32 device tensor with one entry per Gaussian."""
    if not isinstance(filter_3d, torch.Tensor):
        raise ValueError(f"filter_3d must be a torch tensor (got {type(filter_3d).__name__}): compute_filter_3d returns one")
    if filter_3d.dtype != torch.float32:
        raise ValueError(f"filter_3d must be float32 (got {filter_3d.dtype})")
    if not filter_3d.is_cuda:
        raise ValueError("filter_3d must live on the GPU (device tensor)")
    n = int(np.prod(np.shape(means3D))) // 3
    if filter_3d.dim() != 1 or filter_3d.shape[0] != n:
        raise ValueError(f"filter_3d must have shape ({n},), one entry per Gaussian (got {tuple(filter_3d.shape)})")
    if not filter_3d.is_contiguous() or filter_3d.data_ptr() % 16:
        raise ValueError("filter_3d must be contiguous and 16-byte aligned")
    return filter_3d


def apply_filter_3d(scales, opacity, filter_3d, out=None):
    """(s', opacity') = the map of gsr_filter3d.h, as new (N, 3) and (N,) tensors or into `out` = (scales_out, opacity_out).  Rows
    with filter_3d == 0 come back bit for bit."""
    L = _lib.lib()
    dev = _host.device_of(filter_3d, scales, opacity)
    sc = _host.to_dev(scales, torch.float32, dev, (-1, 3))
    op = _host.to_dev(opacity, torch.float32, dev, (-1,))
    N = sc.shape[0]
    f = check_filter_3d(filter_3d, sc)
    if op.shape[0] != N:
        raise ValueError("scales and opacity disagree on the number of Gaussians")
    if out is None:
        out = torch.empty((N, 3), dtype=torch.float32, device=dev), torch.empty((N,), dtype=torch.float32, device=dev)
    so, oo = out
    _args.check_out(so, (N, 3), "scales_out", dev=dev), _args.check_out(oo, (N,), "opacity_out", dev=dev)
    with _host.on_device(dev):
        _lib.check(L.gsr_filter3d_apply(N, _host.ptr(sc), _host.ptr(op), _host.ptr(f), _host.ptr(so), _host.ptr(oo), _host.raw_stream(dev)))
    _host.written_in_place(so, oo)
    return so, oo


def filter_3d_backward(scales, opacity, filter_3d, dL_dscale, dL_dopacity, out=None):
    """The transpose: `dL_dscale` (N, 3) / `dL_dopacity` (N,) are the gradients with respect to (s', opacity'); the result is the
    gradient with respect to the raw (scales, opacity).  out=None works IN PLACE on the two device tensors (views of a gradient
    arena qualify) and tells torch so (_host.written_in_place); out = (dL_dscale_out, dL_dopacity_out) leaves the inputs alone."""
    L = _lib.lib()
    dev = _host.device_of(filter_3d, dL_dscale, scales)
    sc = _host.to_dev(scales, torch.float32, dev, (-1, 3))
    op = _host.to_dev(opacity, torch.float32, dev, (-1,))
    N = sc.shape[0]
    f = check_filter_3d(filter_3d, sc)
    if op.shape[0] != N:
        raise ValueError("scales and opacity disagree on the number of Gaussians")
    if out is None:
        gs, go = dL_dscale, dL_dopacity
        _args.check_out(gs, (N, 3), "dL_dscale", dev=dev), _args.check_out(go, (N,), "dL_dopacity", dev=dev)
        so, oo = gs, go
    else:
        gs = _host.to_dev(dL_dscale, torch.float32, dev, (N, 3))
        go = _host.to_dev(dL_dopacity, torch.float32, dev, (N,))
        so, oo = out
        _args.check_out(so, (N, 3), "dL_dscale out", dev=dev), _args.check_out(oo, (N,), "dL_dopacity out", dev=dev)
    with _host.on_device(dev):
        _lib.check(L.gsr_filter3d_backward(N, _host.ptr(sc), _host.ptr(op), _host.ptr(f), _host.ptr(gs), _host.ptr(go), _host.ptr(so), _host.ptr(oo),
                                           _host.raw_stream(dev)))
    _host.written_in_place(so, oo)
    return so, oo


# ---- the keyword of render_gaussians() / backward(): the filtered tensors ride on the frame, as rho of the antialiased mode does ----
def _raw(given, used):
    """How backward() recognises the raw array a frame was rendered from: a torch tensor by its stamp, anything else (it was copied
    to the device) by value against that copy."""
    return _host.stamp(given), None if isinstance(given, torch.Tensor) else used


def tag_frame(conic_opacity, filter_3d, raw_scales, sc, raw_opacity, op, sc_f, op_f):
    """Called by render_gaussians(filter_3d=...): the filtered tensors (sc_f, op_f) the frame was rendered from ride on the frame's
    conic_opacity view, with the stamps (_host.stamp) of the filter tensor, of the view itself and of the raw arrays."""
    conic_opacity._gsr_filter_3d = (sc_f, op_f, _host.stamp(filter_3d), _host.stamp(conic_opacity), _raw(raw_scales, sc), _raw(raw_opacity, op))


def _same(raw, given, dev, shape, what):
    stamp, copy = raw
    if copy is None:      # (a tensor, unwritten: frame_tag has checked its stamp)
        return _host.to_dev(given, torch.float32, dev, shape)
    if isinstance(given, torch.Tensor) or not torch.equal(copy, _host.to_dev(given, torch.float32, dev, shape)):
        raise ValueError(f"backward(filter_3d=...): `{what}` is not the raw array this frame was rendered from")
    return copy


def frame_tag(conic_opacity, filter_3d, scales, opacity):
    """The filtered forward's tag on its conic_opacity view, or an error: a filtered frame and an unfiltered one are never taken
    for each other, nor two filters, and raw tensors written since the render are stale.  Touches neither the library nor the
    GPU.  Returns the tag, or None without the keyword."""
    tag = getattr(conic_opacity, "_gsr_filter_3d", None)
    if filter_3d is None:
        if tag is not None:
            raise ValueError("this frame was rendered with filter_3d: pass the same tensor to backward(filter_3d=...)")
        return None
    if tag is None:
        raise ValueError("backward(filter_3d=...) needs the conic_opacity view of a frame rendered with render_gaussians(filter_3d=...), "
                         "not a copy of it and not an unfiltered frame")
    _, _, f_stamp, rec_stamp, raw_scales, raw_opacity = tag
    if f_stamp[0]() is not filter_3d:
        raise ValueError("backward(filter_3d=...): this frame was rendered with another filter tensor")
    if not _host.unwritten(f_stamp, filter_3d):
        raise ValueError("backward(filter_3d=...): filter_3d was written in place since the render")
    if not _host.unwritten(rec_stamp, conic_opacity):
        raise ValueError("backward(filter_3d=...): the forward's records were written in place after the render")
    for (stamp, copy), given, what in ((raw_scales, scales, "scales"), (raw_opacity, opacity, "opacity")):
        if copy is None and not _host.unwritten(stamp, given):
            raise ValueError(f"backward(filter_3d=...): `{what}` is not the raw tensor this frame was rendered from, or was written in place since")
    return tag


def raw_inputs(tag, scales, opacity, dev, N):
    """(raw scales, raw opacity) as device tensors for the transpose, checked against what the frame was rendered from."""
    return _same(tag[4], scales, dev, (-1, 3), "scales"), _same(tag[5], opacity, dev, (-1,), "opacity")
