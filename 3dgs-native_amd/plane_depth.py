"""
The ray-plane intersection depth over the lists of a rendered frame (include/gsr_plane_depth.h) over the MI355X library: the depth
model of PGSR, RaDe-GS and GOF.  The forward's depth image, the median depth and the distortion term take a Gaussian for a
fronto-parallel card at 1 / z of its centre; here a flat Gaussian is a piece of its plane, and each pixel blends the inverse depth at
which its own ray meets that plane, m_k(p) = invd_k + gx_k (p.x - x_k) + gy_k (p.y - y_k).

    image, depth, buffers = render_gaussians(...)                        # any rasterize_mode, with or without filter_3d
    n = normal_render.gaussian_normals(scales, rotations, positions, camera)
    s = plane_slopes(n, scales, positions, camera)                       # (N, 2) float32 (gx, gy); (0, 0) where the Gaussian falls back
    pd = render_plane_depth(s, buffers, H, W)                            # (H, W): sum_k w_k m_k, inverse depth x coverage like `depth`
    z = tsdf.depth_from_buffers(pd, buffers["final_Ts"])                 # (H, W) view depth for TSDF fusion
    grads = backward(..., dL_dplane_depth=g, plane_slopes=s, plane_depth_image=pd, gaussian_normals=n)

Under the median rule (include/gsr_plane_median.h: the plane of the ONE Gaussian at which the transmittance falls through one half, the
depth RaDe-GS and GOF fuse) the image and its gradient need no stage of backward():

    med, contrib = render_plane_median_depth(s, buffers, H, W)           # (H, W) float32 1 / depth and (H, W) int32 list position
    z = median_depth.view_depth(med, buffers["final_Ts"])                # (H, W) view depth for TSDF fusion
    grads = backward_view(params, camera, bg, buffers, dL_dpixels)       # the step's other terms
    plane_median_gradients(params, camera, buffers, g, contrib, s, n, grads=grads)     # ADDS into grads["dL_dmean3D"], grads["dL_drot"]

A Gaussian falls back to its centre depth when its normal is zero, it lies at or behind the near plane, the ray to its centre grazes
its plane, or it is not flat (smallest scale above half the middle one).  The image drops in wherever the forward's depth image
does: loss.depth_loss_and_gradient, loss.normal_consistency_loss_and_gradients.  The forward gives the same bits every call.  Its
gradient is a stage of backward() between the blend half and the per-Gaussian half (backward.py), like the normal image's.  `camera`: a
dict with world_to_camera (4 x 4, row-vector convention), tan_fovx, tan_fovy, width and height.  A capacity-mode frame is to be used
only once rendered_count(buffers) has said that it did not overflow.  Everything is enqueued on the current stream; nothing is read
back.
"""
import torch

from . import _args, _frame, _host, _lib
from . import normal_render as _normal_render


def _check_gaussians(normals, scales, means, who):
    """Three float32 device tensors (N, 3); returns N."""
    for name, t in (("normals", normals), ("scales", scales), ("means", means)):
        if not (_args.is_dev(t, torch.float32) and t.dim() == 2 and t.shape[1] == 3):
            raise ValueError(f"{who}: {name} must be a float32 device tensor of shape (N, 3)")
    N = int(normals.shape[0])
    if int(scales.shape[0]) != N or int(means.shape[0]) != N:
        raise ValueError(f"{who}: normals, scales and means disagree on the number of Gaussians")
    return N


def plane_slopes(normals, scales, means, camera, out=None):
    """(N, 2) float32 (gx, gy): the change of a Gaussian's plane's inverse depth per pixel step in x and y, from its camera-space
    normal (normal_render.gaussian_normals), its scales (the raw ones under filter_3d) and its centre; exactly (0, 0) where the
    Gaussian falls back to its centre depth.  `out`: a caller-owned (N, 2) tensor to write into."""
    who = "plane_slopes"
    N = _check_gaussians(normals, scales, means, who)
    tx, ty, W, H = _args.camera_params(camera, who)
    vp, keep = _normal_render.view_floats(camera, who)
    if out is not None:
        _args.check_out(out, (N, 2), "out")
    _args.check_one_device(normals, scales, means, out)
    dev = normals.device
    if out is None:
        out = torch.empty((N, 2), dtype=torch.float32, device=dev)
    if N == 0:
        return out
    L = _lib.lib()
    n, sc, mu = (_host.to_dev(t, torch.float32, dev) for t in (normals, scales, means))
    with _host.on_device(dev):
        _lib.check(L.gsr_plane_slopes(N, _host.ptr(n), _host.ptr(sc), _host.ptr(mu), vp, tx, ty, W, H, _host.ptr(out), _host.raw_stream(dev)))
    _host.written_in_place(out)
    return out


def plane_slopes_backward(dL_dplane_moments, normals, scales, means, camera, dL_dmean3D=None, out=None):
    """(dL_dmean3D, dL_dnormals): ADDS the means' share of the gradient of render_plane_depth through plane_slopes and the staged
    centre to `dL_dmean3D` (N, 3) (None: a fresh zero tensor) and WRITES dL/d(normals) (N, 3) (`out`, or a fresh tensor), from the
    (N, 3) moments backward() returns as `dL_dplane_moments`.  The branch of every Gaussian is held constant."""
    who = "plane_slopes_backward"
    N = _check_gaussians(normals, scales, means, who)
    tx, ty, W, H = _args.camera_params(camera, who)
    vp, keep = _normal_render.view_floats(camera, who)
    if not (_args.is_dev(dL_dplane_moments, torch.float32) and tuple(dL_dplane_moments.shape) == (N, 3) and dL_dplane_moments.is_contiguous()):
        raise ValueError(f"{who}: dL_dplane_moments must be a contiguous float32 device tensor of shape (N, 3)")
    if dL_dmean3D is not None:
        _args.check_out(dL_dmean3D, (N, 3), "dL_dmean3D")
    if out is not None:
        _args.check_out(out, (N, 3), "out")
    _args.check_one_device(normals, scales, means, dL_dplane_moments, dL_dmean3D, out)
    dev = normals.device
    if dL_dmean3D is None:
        dL_dmean3D = torch.zeros((N, 3), dtype=torch.float32, device=dev)
    if out is None:
        out = torch.empty((N, 3), dtype=torch.float32, device=dev)
    if N == 0:
        return dL_dmean3D, out
    L = _lib.lib()
    n, sc, mu, g = (_host.to_dev(t, torch.float32, dev) for t in (normals, scales, means, dL_dplane_moments))
    with _host.on_device(dev):
        _lib.check(L.gsr_plane_slopes_backward(N, _host.ptr(n), _host.ptr(sc), _host.ptr(mu), vp, tx, ty, W, H, _host.ptr(g),
                                               _host.ptr(dL_dmean3D), _host.ptr(out), _host.raw_stream(dev)))
    _host.written_in_place(dL_dmean3D)
    _host.written_in_place(out)
    return dL_dmean3D, out


def check_slopes(slopes, N):
    if not (_args.is_dev(slopes, torch.float32) and tuple(slopes.shape) == (N, 2) and slopes.is_contiguous() and slopes.data_ptr() % 16 == 0):
        raise ValueError("slopes must be a contiguous, 16-byte aligned float32 device tensor of shape (N, 2) with N the frame's number of "
                         "Gaussians (plane_slopes()'s result)")


def render_plane_depth(slopes, buffers, image_height, image_width, out=None, use_block_masks=True):
    """(H, W) float32: out[y, x] = sum over the pixel's contributing list entries of w_k * m_k(p), front to back, one fused
    multiply-add per term, m_k the plane's inverse depth at the pixel held to [invd_k / 4, 4 invd_k]: an inverse depth times coverage,
    what the forward's depth image is for centre depths.  At slopes 0 it is bit for bit features.render_features(invd[:, None]).  `out`:
    a caller-owned tensor to write into (every element is written).  use_block_masks=False walks without the forward's block masks
    (the same bits either way)."""
    fr = _frame.Frame.from_buffers(buffers, image_height, image_width, use_block_masks, inv_depth=True)
    check_slopes(slopes, fr.N)
    out, = fr.outputs(out, [(fr.H, fr.W)], (slopes,))
    if fr.N == 0:
        return out.zero_()
    fr.launch("gsr_plane_depth_forward", _host.ptr(slopes), _host.ptr(out), written=(out,))
    return out


def render_view_plane_depth(params, camera, buffers):
    """(pd, slopes, normals) of a frame forward.render_view() drew from `params` (positions, scales, rotations): the three calls of the
    module's head in one."""
    n = _normal_render.gaussian_normals(params["scales"], params["rotations"], params["positions"], camera)
    s = plane_slopes(n, params["scales"], params["positions"], camera)
    return render_plane_depth(s, buffers, camera["height"], camera["width"]), s, n


# ---- the plane depth under the median rule (include/gsr_plane_median.h) ----
def render_plane_median_depth(slopes, buffers, image_height, image_width, out=None, use_block_masks=True):
    """(med, contrib): (H, W) float32, the inverse depth at which the pixel's ray meets the plane of the ONE Gaussian at which the
    transmittance falls through one half (median_depth's rule, m_k(p) of render_plane_depth held to [invd_k / 4, 4 invd_k]), and
    (H, W) int32, that Gaussian's 1-based position in the tile's list -- bit for bit median_depth.render_median_depth's second result;
    0 and a value of 0 where no entry was applied.  At slopes 0 `med` is bit for bit that call's first result.
    median_depth.view_depth(med, final_Ts) turns it into view depth for TSDF fusion.  `out`: a caller-owned pair to write into (every
    element is written).  use_block_masks=False walks without the forward's block masks (the same bits either way)."""
    fr = _frame.Frame.from_buffers(buffers, image_height, image_width, use_block_masks, inv_depth=True)
    check_slopes(slopes, fr.N)
    med, contrib = fr.outputs(out, [(fr.H, fr.W), (fr.H, fr.W)], (slopes,), pair="(plane_median_inv_depth, plane_median_contrib)",
                              dtypes=(torch.float32, torch.int32))
    if fr.N == 0:
        return med.zero_(), contrib.zero_()
    fr.launch("gsr_pmed_forward", _host.ptr(slopes), _host.ptr(med), _host.ptr(contrib), written=(med, contrib))
    return med, contrib


def plane_median_depth_backward(dL_dmedian, contrib, slopes, buffers, image_height, image_width, out=None, accumulate=False):
    """dL_dplane_moments (N, 3) float32: per pixel whose chosen entry is not clamped, (g, g (p.x - x_k), g (p.y - y_k)) with
    g = dL_dmedian[p], summed over the pixels that chose Gaussian k -- the moments plane_slopes_backward consumes, with weight 1 at the
    chosen entry where backward()'s plane stage has w.  `contrib`: render_plane_median_depth's second result.  `out`: a caller-owned
    (N, 3) tensor; it is cleared first unless accumulate=True, which ADDS into it (backward()'s `dL_dplane_moments`, say: everything
    behind the moments is linear in them, so the two plane terms can share one buffer)."""
    fr = _frame.Frame.from_buffers(buffers, image_height, image_width, False, inv_depth=True)
    check_slopes(slopes, fr.N)
    if not (_args.is_dev(dL_dmedian, torch.float32) and tuple(dL_dmedian.shape) == (fr.H, fr.W) and dL_dmedian.is_contiguous()
            and dL_dmedian.data_ptr() % 16 == 0):
        raise ValueError(f"dL_dmedian must be a contiguous, 16-byte aligned float32 device tensor of shape ({fr.H}, {fr.W})")
    if not (_args.is_dev(contrib, torch.int32) and tuple(contrib.shape) == (fr.H, fr.W) and contrib.is_contiguous() and contrib.data_ptr() % 16 == 0):
        raise ValueError(f"contrib must be a contiguous, 16-byte aligned int32 device tensor of shape ({fr.H}, {fr.W}) "
                         "(render_plane_median_depth()'s second result)")
    if accumulate and out is None:
        raise ValueError("accumulate=True needs out, the (N, 3) tensor to add into")
    out, = fr.outputs(out, [(fr.N, 3)], (slopes, dL_dmedian, contrib))
    if not accumulate:
        out.zero_()
    if fr.N == 0:
        return out
    fr.launch("gsr_pmed_backward", _host.ptr(slopes), _host.ptr(dL_dmedian), _host.ptr(contrib), _host.ptr(out), written=(out,))
    return out


def plane_median_gradients(params, camera, buffers, dL_dmedian, contrib, slopes, normals, grads=None):
    """(dL_dmean3D, dL_drot, moments): the gradient of sum_p dL_dmedian[p] med[p] (render_plane_median_depth) with respect to the
    positions and rotations of `params`, in three calls -- plane_median_depth_backward, plane_slopes_backward,
    normal_render.gaussian_normals_backward -- which ADD into grads["dL_dmean3D"] and grads["dL_drot"] of a backward_view result (so the
    term joins a step's other gradients after backward_view), or into fresh zero tensors.  The median's choice, every Gaussian's branch
    and the clamp are held constant; no stage of backward() is involved."""
    H, W = camera["height"], camera["width"]
    dmean = drot = None
    if grads is not None:
        if not (isinstance(grads, dict) and "dL_dmean3D" in grads and "dL_drot" in grads):
            raise ValueError("grads must be a backward_view() result (a dict with dL_dmean3D and dL_drot) or None")
        dmean, drot = grads["dL_dmean3D"], grads["dL_drot"]
    moments = plane_median_depth_backward(dL_dmedian, contrib, slopes, buffers, H, W)
    dmean, dn = plane_slopes_backward(moments, normals, params["scales"], params["positions"], camera, dL_dmean3D=dmean)
    drot = _normal_render.gaussian_normals_backward(dn, params["scales"], params["rotations"], params["positions"], camera, dL_drot=drot)
    return dmean, drot, moments


def render_view_plane_median_depth(params, camera, buffers):
    """(med, contrib, slopes, normals) of a frame forward.render_view() drew from `params` (positions, scales, rotations)."""
    n = _normal_render.gaussian_normals(params["scales"], params["rotations"], params["positions"], camera)
    s = plane_slopes(n, params["scales"], params["positions"], camera)
    return render_plane_median_depth(s, buffers, camera["height"], camera["width"]) + (s, n)


def check_gradient_triple(dL_dplane_depth, plane_slopes, plane_depth_image, gaussian_normals):
    """backward()'s three keywords: all or none, and with them gaussian_normals."""
    given = [x is not None for x in (dL_dplane_depth, plane_slopes, plane_depth_image)]
    if any(given) and not all(given):
        raise ValueError("backward() needs dL_dplane_depth, plane_slopes and plane_depth_image together: the slopes are plane_slopes()'s "
                         "result, the image render_plane_depth()'s")
    if all(given) and gaussian_normals is None:
        raise ValueError("backward(dL_dplane_depth=...) needs gaussian_normals: the normals plane_slopes() was called with")
    return all(given)
