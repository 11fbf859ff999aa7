"""
Surface normals from the rendered depth (include/gsr_normals.h) over the MI355X library: the unit cross product of the central
differences of the camera-space points P = z r, z = (1 - final_Ts) / depth (`depth` is the forward's expected INVERSE depth), and
the exact gradient of any loss on those normals back to the two images backward() accepts.

    image, depth, buffers = render_gaussians(...)
    normals, valid = normals_from_depth(depth, buffers["final_Ts"], camera)           # (H, W, 3), (H, W) 0 / 1; camera space, facing the camera
    gD, gA = normals_from_depth_backward(dL_dnormals, depth, buffers["final_Ts"], camera)
    grads = backward(..., dL_ddepth_image=gD, dL_dalpha_image=gA)
    normals = depth_to_normals(depth, final_Ts, camera)                                # the same, differentiable in depth and final_Ts

`camera`: a dict with tan_fovx, tan_fovy, width and height (cameras.nerf_camera's).  The cosine loss against a normal prior is
loss.normal_loss_and_gradients.  Gather only: no float atomics, the same bits every call.  Everything is enqueued on the current
stream; nothing is read back.
"""
import numpy as np
import torch

from . import _args, _host, _lib


def pixel_rays(camera):
    """(H, W, 3) float64 numpy: the ray r = (((2x + 1) / W - 1) tan_fovx, ((2y + 1) / H - 1) tan_fovy, 1) of every pixel, the inverse
    of the forward's pixel convention (integer pixel coordinates are the sample positions).  depth z along +z of the camera puts
    the pixel's point at z r."""
    tx, ty, W, H = _args.camera_params(camera, "pixel_rays")
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    r = np.ones((H, W, 3))
    r[..., 0] = (((2.0 * x + 1.0) / W - 1.0) * tx)[None, :]
    r[..., 1] = (((2.0 * y + 1.0) / H - 1.0) * ty)[:, None]
    return r


def normals_from_depth(depth, final_Ts, camera, alpha_min=_lib.NORMALS_ALPHA_MIN):
    """(normals (H, W, 3), valid (H, W)) float32 device tensors: the camera-space unit normal of every pixel whose own and whose
    four neighbours' coverage 1 - final_Ts is at least alpha_min (and whose inverse depth is positive), (0, 0, 0) and valid = 0
    elsewhere.  A fronto-parallel surface gives (0, 0, -1)."""
    who = "normals_from_depth"
    tx, ty, W, H = _args.camera_params(camera, who)
    a = _args.finite(alpha_min, f"{who}: alpha_min")
    _args.image_hw(depth, f"{who}: depth", (H, W))
    _args.image_hw(final_Ts, f"{who}: final_Ts", (H, W))
    L = _lib.lib()
    dev = _host.device_of(depth, final_Ts)
    d = _host.to_dev(depth, torch.float32, dev, (H, W))
    t = _host.to_dev(final_Ts, torch.float32, dev, (H, W))
    normals = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    valid = torch.empty((H, W), dtype=torch.float32, device=dev)
    with _host.on_device(dev):
        _lib.check(L.gsr_normals_from_depth(_host.ptr(d), _host.ptr(t), tx, ty, W, H, a, _host.ptr(normals), _host.ptr(valid), _host.stream_ptr(dev)))
    return normals, valid


def normals_from_depth_backward(dL_dnormals, depth, final_Ts, camera, alpha_min=_lib.NORMALS_ALPHA_MIN):
    """(dL_ddepth_image, dL_dalpha_image), (H, W) float32 each: the exact gradient of a loss with dL/dnormals = `dL_dnormals`
    (H, W, 3) with respect to the inverse-depth image and to the alpha image 1 - final_Ts, for the validity pattern of the call.
    Rows of dL_dnormals at pixels that are not valid are ignored.  Both go straight into backward()."""
    who = "normals_from_depth_backward"
    tx, ty, W, H = _args.camera_params(camera, who)
    a = _args.finite(alpha_min, f"{who}: alpha_min")
    _args.image_hw(depth, f"{who}: depth", (H, W))
    _args.image_hw(final_Ts, f"{who}: final_Ts", (H, W))
    _args.image_hw(dL_dnormals, f"{who}: dL_dnormals", (H, W), 3)
    L = _lib.lib()
    dev = _host.device_of(depth, final_Ts, dL_dnormals)
    d = _host.to_dev(depth, torch.float32, dev, (H, W))
    t = _host.to_dev(final_Ts, torch.float32, dev, (H, W))
    g = _host.to_dev(dL_dnormals, torch.float32, dev, (H, W, 3))
    gD = torch.empty((H, W), dtype=torch.float32, device=dev)
    gA = torch.empty((H, W), dtype=torch.float32, device=dev)
    with _host.on_device(dev):
        stream = _host.stream_ptr(dev)
        ws = _host.workspace("normals", L.gsr_normals_workspace_bytes(W, H), dev, stream)
        _lib.check(L.gsr_normals_from_depth_backward(_host.ptr(d), _host.ptr(t), tx, ty, W, H, a, _host.ptr(g), _host.ptr(gD), _host.ptr(gA),
                                                     _host.ptr(ws), ws.numel(), stream))
    return gD, gA


class _DepthToNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, final_Ts, camera, alpha_min):
        ctx.call = (depth.detach(), final_Ts.detach(), camera, alpha_min)
        return normals_from_depth(ctx.call[0], ctx.call[1], camera, alpha_min)[0]

    @staticmethod
    @torch.autograd.function.once_differentiable      # the library call is a constant to autograd: a double backward is refused
    def backward(ctx, dL_dnormals):
        depth, final_Ts, camera, alpha_min = ctx.call
        gD, gA = normals_from_depth_backward(dL_dnormals.contiguous(), depth, final_Ts, camera, alpha_min)
        # final_Ts = 1 - alpha: the gradient with respect to final_Ts is the negated alpha gradient
        return (gD.view(depth.shape) if ctx.needs_input_grad[0] else None, (-gA).view(final_Ts.shape) if ctx.needs_input_grad[1] else None,
                None, None)


def depth_to_normals(depth, final_Ts, camera, alpha_min=_lib.NORMALS_ALPHA_MIN):
    """normals_from_depth()'s normals as a torch.autograd.Function, differentiable in `depth` and `final_Ts` (device tensors): any
    torch loss on the normals reaches the two images.  d/d(depth) is normals_from_depth_backward's first image bit for bit;
    d/d(final_Ts) is its second NEGATED (the alpha image is 1 - final_Ts); feed backward() from normals_from_depth_backward."""
    tx, ty, W, H = _args.camera_params(camera, "depth_to_normals")
    _args.finite(alpha_min, "depth_to_normals: alpha_min")
    for name, t in (("depth", depth), ("final_Ts", final_Ts)):
        if not _args.is_dev(t, torch.float32):
            raise ValueError(f"depth_to_normals: {name} must be a float32 device tensor")
        _args.image_hw(t, f"depth_to_normals: {name}", (H, W))
    return _DepthToNormals.apply(depth, final_Ts, camera, float(alpha_min))
