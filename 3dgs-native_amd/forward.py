"""
render_gaussians(): the reference's forward call surface (reference forward.py:629-894) over the
MI355X library.  Same keyword arguments, same (image, depth, dict) return with the same dict keys;
arrays come back as torch tensors on the GPU instead of wp.array (callers do `.cpu().numpy()`).
"""
import ctypes as C
import operator
import os

import torch

from . import _host, _lib
from . import filter3d as _filter3d
from .config import TILE_M, TILE_N

# Training use (the default): the forward blend kernel's spare workgroups clear the accumulators of the backward workspace while
# that kernel drains, so the backward() that follows does not start with a 64-byte-per-Gaussian clear of its own.  A render-only
# user can switch it off (it allocates the backward's scratch): forward.PRECLEAR_BACKWARD = False.
# It is lazy: nothing is allocated or cleared for the backward until this process has called backward() once (a render-only
# process never pays for it); the first training step's backward clears for itself.
PRECLEAR_BACKWARD = not bool(int(os.environ.get("GSR_NO_PRECLEAR", "0")))
_backward_seen = False          # set by backward.backward()


def render_gaussians(background, means3D, colors=None, opacity=None, scales=None, rotations=None, scale_modifier=1.0,
                     viewmatrix=None, projmatrix=None, tan_fovx=0.5, tan_fovy=0.5, image_height=256, image_width=256,
                     sh=None, degree=3, campos=None, prefiltered=False, antialiasing=False, clamped=True, debug=False, *,
                     capacity=None, capacity_hint=None, capacity_buffers=None, rasterize_mode="classic", filter_3d=None):
    """Render 3D Gaussians.  `colors`, `prefiltered`, `antialiasing` are accepted and ignored exactly as in
    the reference.  Returns (image (H,W,3) f32, inverse-depth (H,W) f32, buffers).

    rasterize_mode="antialiased" (include/gsr_antialias.h) is the live switch: every Gaussian is drawn with opacity * rho,
    rho = sqrt(max(0.000025, det(Sigma2D) / det(Sigma2D + 0.3 I))), so a sub-pixel Gaussian keeps its energy under the 0.3-pixel
    blur.  The dict has the same twelve keys; `conic_opacity[:, 3]` is then the effective opacity, and rho rides on that view
    (a private tag) for backward(rasterize_mode="antialiased").

    filter_3d=f (include/gsr_filter3d.h; filter3d.compute_filter_3d) renders the scene under Mip-Splatting's 3D smoothing filter:
    exactly the call with filter3d.apply_filter_3d(scales, opacity, f) in place of (scales, opacity) -- scale_modifier applies
    after the filter.  The filtered tensors ride on the conic_opacity view (a private tag) for backward(filter_3d=f), which takes
    the RAW scales and opacity again.  None is the unfiltered call.

    capacity=K (an int, 0 <= K <= 2^30) selects capacity mode (include/gsr_capacity.h): the whole forward is enqueued without
    waiting for the pair count D.  `point_list` then has K entries, of which the first D are valid, and the frame is to be
    trusted only once rendered_count(buffers) has said D <= K.  capacity_hint: the last D the caller knows (default K), which
    picks the backward's blend block shape; backward() passes the same value.  capacity_buffers: optional caller-owned
    {"point_list": int32 [K], "block_masks": uint8 view [K] of >= K + 16 bytes, "binning_ws": uint8 >= gsr_binning_workspace_bytes}."""
    antialiased = _lib.check_rasterize_mode(rasterize_mode)
    if filter_3d is not None:
        _filter3d.check_filter_3d(filter_3d, means3D)
    if capacity is not None:
        capacity, capacity_hint = _check_capacity(capacity, capacity_hint)
    L = _lib.lib()
    dev = _host.device_of(means3D, sh, opacity, scales, rotations)
    if filter_3d is not None:
        # substitution, exactly: from here on `scales` / `opacity` are the filtered device tensors, and everything below -- the tags
        # of the antialiased mode and of the Sigma3D recompute included -- is what a caller who passed them would get
        raw = (scales, _host.to_dev(scales, torch.float32, dev, (-1, 3)), opacity, _host.to_dev(opacity, torch.float32, dev, (-1,)))
        scales, opacity = _filter3d.apply_filter_3d(raw[1], raw[3], filter_3d)
    H, W = int(image_height), int(image_width)
    f32, i32 = torch.float32, torch.int32
    means = _host.to_dev(means3D, f32, dev, (-1, 3))
    N = means.shape[0]
    shs = _host.to_dev(sh, f32, dev, (-1, 3))                 # reference forward.py:687
    if shs.shape[0] != N * 16:
        raise ValueError(f"sh must hold 16 coefficients per Gaussian (got {shs.shape[0]} rows for N={N})")
    op = _host.to_dev(opacity, f32, dev, (-1,))               # (N,1) -> (N,)  utils/wp_utils.py:42-43
    sc = _host.to_dev(scales, f32, dev, (-1, 3))
    rot = _host.to_dev(rotations, f32, dev, (-1, 4))
    if not (op.shape[0] == sc.shape[0] == rot.shape[0] == N):
        raise ValueError("means3D, opacity, scales and rotations disagree on the number of Gaussians")
    cam = _host.make_camera(viewmatrix, projmatrix, campos, background, tan_fovx, tan_fovy, W, H)
    gx, gy = (W + TILE_M - 1) // TILE_M, (H + TILE_N - 1) // TILE_N

    scene = _lib.GsrScene(N, _host.ptr(means), _host.ptr(sc), _host.ptr(rot), _host.ptr(op), _host.ptr(shs),
                          int(degree), float(scale_modifier), 1 if clamped else 0)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    radii, tiles_touched, point_offsets = e((N,), i32), e((N,), i32), e((N,), i32)
    # points_xy_image, conic_opacity and colors are COLUMNS of this call's blend records (one 64-byte row per Gaussian: x, y, conic
    # a b c, opacity, r g b, 1/depth -- GsrGeom.blend_records): strided views, so the forward writes those 36 bytes per Gaussian once
    # instead of twice.  `.cpu().numpy()`, indexing and arithmetic work on them as on any tensor; `.contiguous()` gives a packed copy.
    records = e((N, 16), f32)
    xy, conic_opacity, rgb = records[:, 0:2], records[:, 2:6], records[:, 6:9]
    depths, cov3Ds, clamped_state = e((N,), f32), e((N, 6), f32), e((N, 3), f32)
    aa_scale = e((N,), f32) if antialiased else None      # rho per Gaussian (0 where culled); None is the classic mode
    # d(colour)/d(direction), nine floats per Gaussian: what the SH backward needs of the 48 coefficients (GsrGeom.sh_dir_grad).
    # Only worth its 36 bytes per Gaussian when the caller's SH / position tensors can be recognised again by backward(), i.e.
    # when they are device tensors used in place.
    in_place = lambda given, used: isinstance(given, torch.Tensor) and given.is_cuda and given.data_ptr() == used.data_ptr()
    sh_dir = e((N, 9), f32) if (N > 0 and in_place(sh, shs) and in_place(means3D, means)) else None
    geom = _lib.GsrGeom(_host.ptr(radii), _host.ptr(tiles_touched), _host.ptr(point_offsets), None, _host.ptr(depths),
                        _host.ptr(cov3Ds), None, None, _host.ptr(clamped_state), _host.ptr(records), _host.ptr(sh_dir))
    image, depth_image = e((H, W, 3), f32), e((H, W), f32)
    final_Ts, n_contrib = e((H, W), f32), e((H, W), i32)
    img = _lib.GsrImage(_host.ptr(image), _host.ptr(depth_image), _host.ptr(final_Ts), _host.ptr(n_contrib))
    ranges = e((gx * gy, 2), i32)
    stream = _host.raw_stream(dev)

    # One entry point per stage: the _aa exports with aa_scale = NULL are the classic calls (csrc/api.hip).
    with _host.on_device(dev):
        gws = _host.workspace("geom", L.gsr_geom_workspace_bytes(N), dev, stream)
        if capacity is not None:
            point_list, block_masks, block_order, bwd_ws = _forward_capacity(L, scene, cam, geom, img, ranges, gws, point_offsets, N, W, H, dev,
                                                                            stream, capacity, capacity_hint, capacity_buffers or {}, aa_scale)
        else:
            D = C.c_int64(0)
            _lib.check(L.gsr_forward_count_aa(C.byref(scene), C.byref(cam), C.byref(geom), _host.ptr(gws), gws.numel(), C.byref(D),
                                              _host.ptr(aa_scale), stream))
            D = D.value
            if debug:
                print(f"gsr: {W}x{H}, N={N}, D={D}, SH degree {degree}")
            point_list, block_masks, block_order, bwd_ws, binning = _binning_buffers(L, ranges, N, D, W, H, dev, {}, N > 0 and D > 0)
            bws = _host.workspace("bin", L.gsr_binning_workspace_bytes(N, D, W, H), dev, stream)
            _lib.check(L.gsr_forward_render(C.byref(scene), C.byref(cam), C.byref(geom), C.byref(binning), C.byref(img),
                                            _host.ptr(gws), gws.numel(), _host.ptr(bws), bws.numel(), stream))
    # Let a following backward() use what this call derived.  Every tag rides on the tensor backward() is handed anyway (the
    # reference's callers re-pack the dicts by hand, train.py:986-1000) and states "valid while these very tensors are unwritten"
    # as _host.stamp()s, which backward() holds against what it is given with _host.unwritten() -- torch's version counters; the
    # library's own in-place writers, Adam and the opacity reset, bump them too (_host.written_in_place).  Anything else a tag
    # depends on is a plain field of it.
    if N > 0:
        stamp = _host.stamp
        # the records stand in for the three arrays when backward() gets these very views (views share their base's counter, so a
        # write through any of them, or into the records, is seen)
        xy._gsr_records = (records, {"means2D": stamp(xy), "conic_opacity": stamp(conic_opacity), "rgb": stamp(rgb)})
        if sh_dir is not None:
            # the direction derivatives ride on clamped_state (which backward() receives as `clamped`), valid for these very
            # sh / means3D tensors, this camera position and this degree
            clamped_state._gsr_sh_dir = (sh_dir, stamp(sh), stamp(means3D), tuple(cam.campos), int(degree))
        if antialiased:
            # rho rides on the conic_opacity view (column 5 of the records holds opacity * rho), valid while that view is unwritten (the
            # tensor a tag rides on needs no reference to itself: its version alone) and for this opacity: a device tensor used in
            # place by its stamp; anything else, which was copied to the device, by value against that copy.
            # backward(rasterize_mode="antialiased") refuses anything else
            by_value = None if in_place(opacity, op) else op
            conic_opacity._gsr_aa_scale = (aa_scale, *stamp(opacity if by_value is None else None), conic_opacity._version, by_value)
        if filter_3d is not None:
            _filter3d.tag_frame(conic_opacity, filter_3d, *raw, scales, opacity)
        if in_place(scales, sc) and in_place(rotations, rot):
            # backward() need not read cov3Ds back when it is handed this very tensor with these very scales / rotations and the
            # same scale_modifier: the kernel recomputes Sigma3D with the forward's instructions (gsr.h GsrGeom.cov3D)
            cov3Ds._gsr_sigma_of = (stamp(cov3Ds), stamp(scales), stamp(rotations), float(scale_modifier))
        # the block masks, and the block order derived from them, ride on the point_list tensor: they describe these records, up to
        # these n_contrib, so a caller that hands backward() every one of this call's buffers gets the mask-driven compaction,
        # anyone else the self-contained one
        owners = {"ranges": ranges, "n_contrib": n_contrib, "final_Ts": final_Ts, "means2D": xy, "conic_opacity": conic_opacity}
        point_list._gsr_block_masks = (block_masks, {k: stamp(v) for k, v in owners.items()}, block_order)
        if bwd_ws is not None:      # "a backward workspace with clean accumulators": the first backward() handed this point_list takes it
            point_list._gsr_cleared_ws = [bwd_ws, N]
    return image, depth_image, {
        "radii": radii, "point_offsets": point_offsets, "points_xy_image": xy, "depths": depths, "colors": rgb,
        "cov3Ds": cov3Ds, "conic_opacity": conic_opacity, "point_list": point_list, "ranges": ranges,
        "final_Ts": final_Ts, "n_contrib": n_contrib, "clamped_state": clamped_state,
    }


def render_view(params, camera, background, **kw):
    """render_gaussians() of a trainer's parameter dict (positions, scales, rotations, opacities, shs) from a cameras.nerf_camera
    dict at SH degree 3: the key names of the two dicts, nothing else.  The tensors go through as they are (the frame's tags ride
    on them); **kw is render_gaussians' keyword-only part (rasterize_mode, filter_3d, capacity, capacity_hint)."""
    return render_gaussians(background=background, means3D=params["positions"], opacity=params["opacities"], scales=params["scales"],
                            rotations=params["rotations"], viewmatrix=camera["world_to_camera"], projmatrix=camera["full_proj_matrix"],
                            tan_fovx=camera["tan_fovx"], tan_fovy=camera["tan_fovy"], image_height=camera["height"],
                            image_width=camera["width"], sh=params["shs"], degree=3, campos=camera["camera_center"], **kw)


def _check_capacity(capacity, hint):
    """Capacity-mode arguments, checked before anything touches the GPU."""
    out = []
    for name, v in (("capacity", capacity), ("capacity_hint", hint)):
        if v is None and name == "capacity_hint":
            out.append(None)
            continue
        if isinstance(v, bool):
            raise TypeError(f"{name} must be an integer (got bool)")
        try:
            v = operator.index(v)
        except TypeError:
            raise TypeError(f"{name} must be an integer (got {type(v).__name__})") from None
        if not 0 <= v <= _lib.MAX_RENDERED:
            raise ValueError(f"{name} must lie in [0, 2^30] (got {v})")
        out.append(v)
    return out[0], out[1]


def _binning_buffers(L, ranges, N, D, W, H, dev, bufs, preclear):
    """The binning buffers of one forward with room for D pairs, and their GsrBinning: point_list and block_masks (the caller's
    `capacity_buffers`, else fresh), block order, and the pre-cleared backward workspace when `preclear` and the process trains."""
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    point_list = bufs.get("point_list")
    if point_list is None:
        point_list = e((D,), torch.int32)
    # per-entry 8x4-block hit masks: written by the forward blend, read by backward() (allocated with 16 spare bytes: the backward
    # reads them 16 at a time)
    block_masks = bufs.get("block_masks")
    if block_masks is None:
        block_masks = e((D + 16,), torch.uint8)[:D]
    if point_list.numel() < D or block_masks.numel() < D:
        raise ValueError("capacity_buffers: point_list and block_masks need K entries")
    # the backward blend's blocks filed by cost, heaviest first (GsrBinning.block_order): filled by the forward blend from the masks
    block_order = e((int(L.gsr_block_order_ints(W, H)),), torch.int32)
    # The backward's workspace, one per call: its accumulator records are what backward() returns dL_dcolor / dL_dmean2D /
    # dL_dconic as views of, so it must not be shared between calls.  Handed to the forward, its records are cleared by the
    # blend kernel's spare workgroups.
    bwd_ws = None
    if PRECLEAR_BACKWARD and _backward_seen and preclear:
        bwd_ws = e((int(L.gsr_backward_workspace_bytes(N, D, W, H)),), torch.uint8)
    binning = _lib.GsrBinning(D, _host.ptr(point_list), _host.ptr(ranges), _host.ptr(block_masks), _host.ptr(block_order), _host.ptr(bwd_ws), 0)
    return point_list, block_masks, block_order, bwd_ws, binning


def _forward_capacity(L, scene, cam, geom, img, ranges, gws, point_offsets, N, W, H, dev, stream, K, hint, bufs, aa_scale=None):
    """gsr_forward_capacity: buffers for K pairs, no wait for D.  The count is copied (non-blocking) into pinned memory behind an
    event; it rides on the point_list tensor (`_gsr_capacity`) for rendered_count() and backward()."""
    # (D is not known here: the clear is promised for an empty frame too)
    point_list, block_masks, block_order, bwd_ws, binning = _binning_buffers(L, ranges, N, K, W, H, dev, bufs, N > 0)
    # the shape hint: the backward skips its blend for D = 0, so a frame that may hold pairs passes at least 1
    hint = max(1, K if hint is None else hint) if K > 0 else 0
    need = int(L.gsr_binning_workspace_bytes(N, K, W, H))
    bws = bufs.get("binning_ws")
    if bws is None:
        bws = _host.workspace("bin", need, dev, stream)
    elif bws.numel() < need:
        raise ValueError(f"capacity_buffers: binning_ws needs {need} bytes")
    _lib.check(L.gsr_forward_capacity_aa(C.byref(scene), C.byref(cam), C.byref(geom), C.byref(binning), C.byref(img), _host.ptr(gws), gws.numel(),
                                         _host.ptr(bws), bws.numel(), hint, _host.ptr(aa_scale), stream))
    count = torch.zeros((1,), dtype=torch.int32, pin_memory=True)
    if N > 0:
        count.copy_(point_offsets[N - 1:N], non_blocking=True)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(dev))
    point_list._gsr_capacity = (K, hint, count, done)
    return point_list, block_masks, block_order, bwd_ws


def rendered_count(buf):
    """(D, overflowed) of a capacity-mode frame: waits for that frame's count copy only (its event), not for the stream.  `buf`:
    the dict render_gaussians returned, or its point_list.  overflowed = D > K: nothing computed from that frame is trusted."""
    pl = buf["point_list"] if isinstance(buf, dict) else buf
    tag = getattr(pl, "_gsr_capacity", None)
    if tag is None:
        raise ValueError("not a capacity-mode frame: its D is point_list.shape[0]")
    K, _, count, done = tag
    done.synchronize()
    D = int(count[0])
    return D, bool(D < 0 or D > K)
