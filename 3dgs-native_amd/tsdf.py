"""
TSDF fusion of rendered depth into a dense volume and triangle-mesh extraction by marching tetrahedra (include/gsr_tsdf.h) over the
MI355X library: the last step of the geometry workflow -- render depth and colour from the training cameras, fuse, extract.

    vol = TSDFVolume(origin, voxel_size, (Gx, Gy, Gz))                     # origin: the centre of voxel (0, 0, 0)
    image, depth, buffers = render_gaussians(...)
    z = depth_from_buffers(depth, buffers["final_Ts"])                     # (H, W) view depth, 0 = no measurement
    vol.integrate(z, camera, color=image)                                  # or vol.integrate_views(depths, cameras, colors)
    vertices, colors, keys = vol.extract_mesh(min_weight=1.0)              # a triangle soup: (T, 3, 3), (T, 3, 3) or None, (T, 3) int64
    verts, faces, vcolors = weld(vertices, keys, colors)                   # host, numpy: an indexed mesh
    point_cloud.save_mesh_ply("mesh.ply", verts, faces, vcolors)

`camera`: a dict with world_to_camera (4 x 4, row-vector form, translation in row 3), tan_fovx, tan_fovy, width and height
(cameras.nerf_camera's).  Integration is sequential float32 in view order: the same bits however the views are split into calls.
Everything is enqueued on the current stream.  extract_mesh makes ONE host read, of the triangle count, to size its outputs:
extraction is an offline step.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _args, _host, _lib
from . import median_depth as _median_depth
from . import plane_depth as _plane_depth


def check_volume(origin, voxel_size, dims, who="TSDFVolume"):
    """(origin float32 (3,), voxel_size, (Gx, Gy, Gz)), judged before the GPU is touched."""
    try:
        o = np.asarray(origin, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        o = np.zeros(0)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError(f"{who}: origin must be 3 finite numbers, not {origin!r}")
    s = _args.positive(voxel_size, f"{who}: voxel_size")
    try:
        g = tuple(dims)
        ok = len(g) == 3 and all(int(n) == n and 1 <= n <= _lib.TSDF_MAX_DIM for n in g)
    except (TypeError, ValueError):
        ok = False
    if not ok or int(g[0]) * int(g[1]) * int(g[2]) > _lib.TSDF_MAX_VOXELS:
        raise ValueError(f"{who}: dims must be 3 integers in 1 .. {_lib.TSDF_MAX_DIM} with a product <= 2^31, not {dims!r}")
    return o.astype(np.float32), s, (int(g[0]), int(g[1]), int(g[2]))


def check_view_camera(camera, who):
    """(view 16 floats, tan_fovx, tan_fovy, W, H) of a camera dict, judged before the GPU is touched."""
    tx, ty, W, H = _args.camera_params(camera, who)
    try:
        m = np.asarray(camera["world_to_camera"], dtype=np.float64)
    except (KeyError, TypeError, ValueError):
        raise ValueError(f"{who}: camera must hold world_to_camera, a 4 x 4 matrix") from None
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise ValueError(f"{who}: camera world_to_camera must be a finite 4 x 4 matrix")
    return m.astype(np.float32).reshape(16), tx, ty, W, H


def depth_from_buffers(depth_image, final_Ts, alpha_min=_lib.NORMALS_ALPHA_MIN):
    """(H, W) float32 device tensor: the view depth z = (1 - final_Ts) / depth_image (`depth_image` is the forward's expected INVERSE
    depth) where gsr_normals.h defines the pixel -- coverage 1 - final_Ts at least alpha_min, inverse depth positive, both finite --
    and 0 elsewhere.  0 means "no measurement" to the integrator."""
    a = _args.finite(alpha_min, "depth_from_buffers: alpha_min")
    H, W = _args.image_hw(depth_image, "depth_from_buffers: depth_image")
    if H * W > 1 << 28:
        raise ValueError(f"depth_from_buffers: depth_image must have H * W <= 2^28, not {H} x {W}")
    _args.image_hw(final_Ts, "depth_from_buffers: final_Ts", (H, W))
    L = _lib.lib()
    dev = _host.device_of(depth_image, final_Ts)
    d = _host.to_dev(depth_image, torch.float32, dev, (H, W))
    t = _host.to_dev(final_Ts, torch.float32, dev, (H, W))
    z = torch.empty((H, W), dtype=torch.float32, device=dev)
    with _host.on_device(dev):
        _lib.check(L.gsr_tsdf_depth(_host.ptr(d), _host.ptr(t), W, H, a, _host.ptr(z), _host.stream_ptr(dev)))
    return z


class TSDFVolume:
    """A dense truncated-signed-distance volume on the device: `tsdf`, `weight` (Gz, Gy, Gx) and `color` (Gz, Gy, Gx, 3) or None,
    float32.  `origin` is the world position of the centre of voxel (0, 0, 0); `trunc` the truncation distance (4 voxels by
    default); `w_max` caps the accumulated weight (a running average over about w_max views once reached)."""

    def __init__(self, origin, voxel_size, dims, trunc=None, w_max=float("inf"), color=True, device=None):
        self.origin, self.voxel_size, self.dims = check_volume(origin, voxel_size, dims)
        self.trunc = _args.positive(4.0 * self.voxel_size if trunc is None else trunc, "TSDFVolume: trunc")
        self.w_max = _args.positive(w_max, "TSDFVolume: w_max", allow_inf=True)
        L = _lib.lib()
        dev = torch.device(device) if device is not None else _host.device_of()
        if dev.type != "cuda":
            raise ValueError("TSDFVolume: device must be a GPU")
        self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        Gx, Gy, Gz = self.dims
        self.tsdf = torch.empty((Gz, Gy, Gx), dtype=torch.float32, device=self.device)
        self.weight = torch.empty((Gz, Gy, Gx), dtype=torch.float32, device=self.device)
        self.color = torch.empty((Gz, Gy, Gx, 3), dtype=torch.float32, device=self.device) if color else None
        self._ws = torch.empty(max(16, int(L.gsr_mesh_workspace_bytes(Gx, Gy, Gz))), dtype=torch.uint8, device=self.device)
        self._total = torch.empty(1, dtype=torch.int64, device=self.device)
        self.reset()

    def _struct(self):
        v = _lib.GsrTsdfVolume()
        v.Gx, v.Gy, v.Gz = self.dims
        v.voxel_size = self.voxel_size
        v.origin[:] = self.origin.tolist()
        v.tsdf, v.weight, v.color = _host.ptr(self.tsdf), _host.ptr(self.weight), _host.ptr(self.color)
        return v

    def reset(self):
        """tsdf = 1, weight = 0, color = 0."""
        L = _lib.lib()
        with _host.on_device(self.device):
            _lib.check(L.gsr_tsdf_reset(C.byref(self._struct()), _host.stream_ptr(self.device)))
        return self

    def integrate(self, depth, camera, color=None, depth_max=float("inf"), weight=1.0):
        """Fuse one view: `depth` (H, W) view depth (depth_from_buffers'), `color` (H, W, 3) or None."""
        return self.integrate_views([depth], [camera], None if color is None else [color], depth_max=depth_max, weights=weight)

    def integrate_views(self, depths, cameras, colors=None, depth_max=float("inf"), weights=1.0):
        """Fuse V views in the order given, GSR_TSDF_VIEWS_PER_LAUNCH to a launch: the volume is read and written once per launch.
        `colors`: None, or one image or None per view; `weights`: one observation weight, or one per view."""
        who = "integrate_views"
        depths, cameras = list(depths), list(cameras)
        V = len(depths)
        if V < 1 or len(cameras) != V:
            raise ValueError(f"{who}: needs at least one view and as many cameras as depths, not {V} and {len(cameras)}")
        colors = [None] * V if colors is None else list(colors)
        if len(colors) != V:
            raise ValueError(f"{who}: colors must be None or hold one image (or None) per view, not {len(colors)} for {V} views")
        weights = [weights] * V if np.ndim(weights) == 0 else list(weights)
        if len(weights) != V:
            raise ValueError(f"{who}: weights must be one number or one per view, not {len(weights)} for {V} views")
        dmax = _args.positive(depth_max, f"{who}: depth_max", allow_inf=True)
        parsed = []
        for k in range(V):
            view, tx, ty, W, H = check_view_camera(cameras[k], who)
            _args.image_hw(depths[k], f"{who}: depth", (H, W))
            if colors[k] is not None:
                _args.image_hw(colors[k], f"{who}: color", (H, W), 3)
            parsed.append((view, tx, ty, W, H, _args.positive(weights[k], f"{who}: weight")))
        L = _lib.lib()
        dev = self.device
        recs = (_lib.GsrTsdfView * V)()
        keep = []
        for k, (view, tx, ty, W, H, w) in enumerate(parsed):
            d = _host.to_dev(depths[k], torch.float32, dev, (H, W))
            c = None if colors[k] is None else _host.to_dev(colors[k], torch.float32, dev, (H, W, 3))
            keep += [d, c]
            r = recs[k]
            r.depth, r.color = _host.ptr(d), _host.ptr(c)
            r.view[:] = view.tolist()
            r.tan_fovx, r.tan_fovy, r.W, r.H, r.w_obs = tx, ty, W, H, w
        with _host.on_device(dev):
            _lib.check(L.gsr_tsdf_integrate(C.byref(self._struct()), V, recs, self.trunc, dmax, self.w_max, _host.stream_ptr(dev)))
        return self

    def extract_mesh(self, min_weight=1.0):
        """(vertices (T, 3, 3), colors (T, 3, 3) or None, keys (T, 3) int64) device tensors: the triangle soup of the zero level set
        over the cells whose eight corners all have weight >= min_weight, in cell order.  Equal keys are the same vertex, bit for
        bit (weld).  Triangles are wound so that their normals point into free space.  One host read: the count."""
        mw = _args.positive(min_weight, "extract_mesh: min_weight", allow_inf=True)
        L = _lib.lib()
        dev = self.device
        vol = self._struct()
        with _host.on_device(dev):
            stream = _host.stream_ptr(dev)
            _lib.check(L.gsr_mesh_count(C.byref(vol), mw, _host.ptr(self._ws), self._ws.numel(), _host.ptr(self._total), stream))
            T = int(self._total.item())                      # the one host read
            vertices = torch.empty((T, 3, 3), dtype=torch.float32, device=dev)
            colors = torch.empty((T, 3, 3), dtype=torch.float32, device=dev) if self.color is not None else None
            keys = torch.empty((T, 3), dtype=torch.int64, device=dev)
            if T > 0:
                _lib.check(L.gsr_mesh_emit(C.byref(vol), mw, _host.ptr(self._ws), self._ws.numel(), T, _host.ptr(vertices), _host.ptr(colors),
                                           _host.ptr(keys), stream))
        return vertices, colors, keys


def weld(vertices, keys, colors=None):
    """Triangle soup -> indexed mesh, on the host: vertices with equal keys are one vertex (they are equal bit for bit).  Returns
    (verts (N, 3) float32, faces (T, 3) int32, colors (N, 3) float32 or None), vertices in ascending key order."""
    def host(x):
        return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    v, k = host(vertices).astype(np.float32, copy=False), host(keys)
    if v.ndim != 3 or v.shape[1:] != (3, 3) or k.shape != v.shape[:2] or k.dtype.kind not in "iu":
        raise ValueError(f"weld: vertices must have shape (T, 3, 3) and keys (T, 3) integers, not {v.shape} and {k.shape} {k.dtype}")
    if colors is not None and tuple(np.shape(colors)) != v.shape:
        raise ValueError(f"weld: colors must have shape {v.shape}, not {tuple(np.shape(colors))}")
    _, first, inverse = np.unique(k.reshape(-1), return_index=True, return_inverse=True)
    verts = v.reshape(-1, 3)[first]
    faces = inverse.reshape(-1, 3).astype(np.int32)
    cols = None if colors is None else host(colors).astype(np.float32, copy=False).reshape(-1, 3)[first]
    return verts, faces, cols


DEPTH_MODES = ("expected", "median")     # fuse_views(depth_mode=...)


def scene_bounds(cameras):
    """(centre (3,), half_side) of the cube the workflow fuses into when the caller names none: the centre is the point nearest to all
    optical axes (the cameras' common look-at point; their centroid when the axes are parallel), the half side is half of
    densify.calculate_scene_extent of the camera centres -- an object framed by orbiting cameras lies well inside it."""
    from .densify import calculate_scene_extent
    centres = np.stack([np.asarray(c["camera_center"], np.float64).reshape(3) for c in cameras])
    axes = np.stack([np.asarray(c["world_to_camera"], np.float64)[:3, 2] for c in cameras])     # the camera's +z in world space
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    P = np.eye(3)[None] - axes[:, :, None] * axes[:, None, :]                                    # projectors off each axis
    A, b = P.sum(0), np.einsum("nij,nj->i", P, centres)
    centre = np.linalg.solve(A, b) if np.linalg.cond(A) < 1e8 else centres.mean(0)
    return centre, 0.5 * calculate_scene_extent(centres)


def fuse_views(render, cameras, voxel_size=None, resolution=256, centre=None, half_side=None, trunc=None, depth_max=float("inf"), min_weight=1.0,
               alpha_min=_lib.NORMALS_ALPHA_MIN, w_max=float("inf"), device=None, depth_mode="expected", plane_depth=False, params=None):
    """The workflow behind examples/extract_mesh.py and train.py --mesh-out: render every camera (`render(camera)` returns the
    forward's (image, depth, buffers)), fuse depth_from_buffers' depth and the image into a cube of `resolution` voxels per side
    (or of `voxel_size`) around scene_bounds (or `centre`, `half_side`), extract and weld.  Returns (verts, faces, colors, info).
    depth_mode="median" fuses median_depth.view_depth of median_depth.render_median_depth instead: the depth of the Gaussian at which
    the transmittance falls through one half, where "expected" is the blended inverse depth over the coverage.
    plane_depth=True is another axis, the depth MODEL under the expected blend: every view fuses depth_from_buffers of
    plane_depth.render_plane_depth (include/gsr_plane_depth.h: a flat Gaussian contributes the depth at which the pixel's ray meets its
    plane, not the depth of its centre).  plane_depth="median" is that model under the median rule: every view fuses
    median_depth.view_depth of plane_depth.render_plane_median_depth (include/gsr_plane_median.h: the plane of the one Gaussian at which
    the transmittance falls through one half, what RaDe-GS and GOF fuse).  Both need `params`, the dict `render` draws from (positions,
    scales, rotations).  depth_mode stays the CENTRE-depth axis: depth_mode="median" raises with any plane_depth -- the plane depth
    under the median rule is plane_depth="median"."""
    if depth_mode not in DEPTH_MODES:
        raise ValueError(f"fuse_views: depth_mode must be one of {DEPTH_MODES} (got {depth_mode!r})")
    if not (isinstance(plane_depth, bool) or (isinstance(plane_depth, str) and plane_depth == "median")):
        raise ValueError(f"fuse_views: plane_depth must be False, True or 'median' (got {plane_depth!r})")
    if plane_depth and depth_mode != "expected":
        raise ValueError(f"fuse_views: plane_depth={plane_depth!r} does not combine with depth_mode={depth_mode!r}, the centre-depth axis: "
                         "plane_depth=True blends the plane depth under the expected rule, and the plane depth under the median rule is "
                         "plane_depth='median'")
    if plane_depth and not (isinstance(params, dict) and all(k in params for k in ("positions", "scales", "rotations"))):
        raise ValueError(f"fuse_views: plane_depth={plane_depth!r} needs params, the dict with positions, scales and rotations that render() "
                         "draws from")
    cameras = list(cameras)
    if not cameras:
        raise ValueError("fuse_views: needs at least one camera")
    auto_c, auto_h = scene_bounds(cameras)
    centre = auto_c if centre is None else np.asarray(centre, np.float64).reshape(3)
    half = float(auto_h if half_side is None else half_side)
    if voxel_size is None:
        G = int(resolution)
        voxel_size = 2.0 * half / (G - 1) if G > 1 else 2.0 * half
    else:
        G = int(math.ceil(2.0 * half / float(voxel_size))) + 1
    if not 2 <= G <= _lib.TSDF_MAX_DIM or G ** 3 > _lib.TSDF_MAX_VOXELS:
        raise ValueError(f"fuse_views: {G} voxels per side: the resolution must be in 2 .. {_lib.TSDF_MAX_DIM} with a cube of at most 2^31 voxels")
    vol = TSDFVolume(centre - 0.5 * voxel_size * (G - 1), voxel_size, (G, G, G), trunc=trunc, w_max=w_max, device=device)
    for first in range(0, len(cameras), _lib.TSDF_VIEWS_PER_LAUNCH):                              # one launch's views at a time: 16 images resident
        batch = cameras[first:first + _lib.TSDF_VIEWS_PER_LAUNCH]
        depths, colors = [], []
        for c in batch:
            image, depth, buffers = render(c)
            H, W = c["height"], c["width"]
            if plane_depth == "median":
                med = _plane_depth.render_view_plane_median_depth(params, c, buffers)[0]
                depths.append(_median_depth.view_depth(med, buffers["final_Ts"].reshape(H, W), alpha_min))
            elif plane_depth:
                pd =_plane_depth.render_view_plane_depth(params, c, buffers)[0]
                depths.append(depth_from_buffers(pd, buffers["final_Ts"].reshape(H, W), alpha_min))
            elif depth_mode == "median":
                med, _ = _median_depth.render_median_depth(buffers, H, W)
                depths.append(_median_depth.view_depth(med, buffers["final_Ts"].reshape(H, W), alpha_min))
            else:
                depths.append(depth_from_buffers(depth.reshape(H, W), buffers["final_Ts"].reshape(H, W), alpha_min))
            colors.append(image.reshape(H, W, 3))
        vol.integrate_views(depths, batch, colors, depth_max=depth_max)
    vertices, vcolors, keys = vol.extract_mesh(min_weight)
    verts, faces, cols = weld(vertices, keys, vcolors)
    info = {"resolution": G, "voxel_size": float(voxel_size), "trunc": vol.trunc, "centre": [float(x) for x in centre], "half_side": half,
            "views": len(cameras), "triangles": int(len(faces)), "vertices": int(len(verts))}
    if depth_mode != "expected":
        info["depth_mode"] = depth_mode
    if plane_depth:
        info["plane_depth"] = plane_depth
    return verts, faces, cols, info
