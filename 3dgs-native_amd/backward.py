"""
backward(): the reference's gradient call surface (reference backward.py:955-1196) over the MI355X
library.  Same keyword arguments and the same nine-key return dict (`dL_dcov3D` is all zeros, as in
the reference, whose real dL/dSigma3D is a local that never leaves backward_preprocess, :812/:1119).
The five optimizer gradients are views into one flat float32 arena (`_arena`, 59 floats per
Gaussian: mean3D | scale | rot | opacity | shs, each segment padded to a multiple of 4 floats, dist.arena_offsets) so
data-parallel training reduces them with a single RCCL all-reduce.

One keyword beyond the reference's: `sh_gradient="factored"` (view-parallel training, dist.py) leaves the 48-float SH
gradient unwritten and returns instead the 3-float colour gradient it is an outer product of, as a self-contained view
payload (`_view_payload`: N rows, then the camera position); `_arena` is then the 11 floats mean3D | scale | rot | opacity
and `dL_dshs` is None until `dist.sh_gradients_from_views` rebuilds it from all views' payloads ("both" returns the dense
arena and the payload of the same call).  `on_payload(payload)` is called as soon as the payload is complete -- after the
blend half, before the per-Gaussian half -- so an exchange can start early (dist.FactoredExchange).

Two more keywords (include/gsr_aux_grads.h): `dL_ddepth_image` and `dL_dalpha_image`, (H, W) gradients with respect to the
forward's inverse-depth image (img_buffer "depth_image") and its alpha image 1 - final_Ts.  With either, the call runs the
auxiliary backward (dL_dpixels may then be None), and the result has one more key, `dL_dinv_depths`: dL/d(1/depth) per
Gaussian, an (N,) strided view of the accumulator records.  With neither, the call is exactly the one above.

`camera_grad=True` (include/gsr_camera_grads.h) adds three keys: `dL_dviewmatrix` (4, 4), `dL_dprojmatrix` (4, 4) and
`dL_dcampos` (3,), float32 device tensors, the true derivative of the forward with respect to `viewmatrix`, `projmatrix` and
`campos`, each taken as independent, in the row-vector convention p_view = [p, 1] @ viewmatrix.  They are summed by one more
kernel pair after the backward above, which reads its accumulators and writes nothing else, so every other key is what the
call with camera_grad=False returns.  The sum is bitwise reproducible for given accumulators.  pose.pose_gradient turns the
three into the gradient of a per-view pose correction.

`absgrad=True` (include/gsr_densify_stats.h, GSR_BWD_ABSGRAD) adds one key, `dL_dmean2D_abs`: an (N, 2) strided view of columns
12-13 of the accumulator records, the sums of the MAGNITUDES of the per-(pixel, entry) terms whose signed sums are
dL_dmean2D[:, 0:2] (AbsGS).  The flag rides on the one entry point every call runs (gsr_backward_aa); every other key is what the call without it returns, up to
float-atomic order.  Without the keyword the two columns are zero and the key is absent.  Either way the returned `dL_dmean2D`
carries a private tag (`_gsr_backward_ws`: workspace, its version counter, whether the absolute columns were filled) through
which densify.DensifyStats.update finds the accumulators.

`filter_3d=f` (include/gsr_filter3d.h) is the backward of a frame rendered with render_gaussians(filter_3d=f): `scales` and `opacity`
are the RAW parameters again, unwritten since the render, `f` the very tensor, unwritten too, and `conic_opacity` that frame's own
view.  The call is the backward of the filtered scene (the frame carries its tensors) followed by the transpose of the map
(filter3d.filter_3d_backward, in place in the arena): dL_dscale and dL_dopacity come back with respect to the raw parameters, every
other key is the filtered scene's.  Anything else raises, as for the antialiased mode, with which it composes, as with every other keyword.

`rasterize_mode="antialiased"` (include/gsr_antialias.h) is the backward of a frame rendered with that mode: `conic_opacity` must
be that frame's own view, unwritten, and `opacity` the opacity it was rendered from, unwritten (render_gaussians leaves rho on the
view as a private tag).  dL_dopacity is then rho times the blend stage's gradient, and the derivative of rho joins dL_dmean3D,
dL_dscale, dL_drot and, with camera_grad, the camera gradient.  Without a valid tag the call raises: there is nothing to fall back
to, and classic gradients for an antialiased frame would be silently wrong; an antialiased frame handed to the default
`rasterize_mode="classic"` raises for the same reason.  It composes with every keyword above and with capacity frames.

`dL_ddistortion=g, distortion_moments=moments` (include/gsr_distortion.h; both or neither) add the gradient of
sum_p g[p] Dist(p), the depth-distortion term of distortion.render_distortion(), whose second result `moments` is.  The call then
always runs in three parts: the blend half, the distortion stage -- which ADDS its screen-space gradients into columns 3-4, 6, 7,
9, 10 and 11 of the accumulator records -- and the AUX per-Gaussian half (gsr_backward_geom_aa), and the result carries
`dL_dinv_depths`.  `dL_ddistortion` alone is legal (dL_dpixels=None: a zero alpha gradient stands in for the blend half's image).
It composes with camera_grad (the camera kernels read the same accumulators), the antialiased mode, filter_3d, capacity frames and
sh_gradient="factored" (the payload is made of the colour columns, which the stage does not touch).  `dL_dmean2D_abs` (columns
12-13) stays the colour, depth and alpha terms' alone: the distortion term does not enter the densification statistic.  Without
the two keywords the call is exactly the one above.

`dL_dnormal_image=gN, gaussian_normals=n, normal_image=nimg` (include/gsr_normal_render.h; all three or none) add the gradient of
sum_p gN[p] . nimg[p], nimg = normal_render.render_normals(n, ...) the blended image of the Gaussians' own normals
n = normal_render.gaussian_normals(...).  The call then runs in three parts as for the distortion term: the blend half, the stage or
stages (the distortion stage first when both are present) -- the normal stage ADDS its screen-space gradients into columns 3-4, 6, 7,
9 and 10 of the accumulator records and writes `dL_dgaussian_normals`, an (N, 3) buffer -- and gsr_backward_geom_aa; the result
carries `dL_dgaussian_normals` and `dL_dinv_depths`.  After the per-Gaussian half gsr_gaussian_normals_backward adds the normals'
gradient to dL_drot, from the scales, rotations, means and viewmatrix AS THE CALLER PASSED THEM (under filter_3d the raw scales: the
map is monotone per axis, so the shortest axis is the same); `normal_param_grad=False` skips that kernel, for callers who blend
normals of their own and want only `dL_dgaussian_normals`.  `dL_dnormal_image` alone is legal (dL_dpixels=None).  It composes with
camera_grad (the screen-space columns only: the normals' direct dependence on viewmatrix is left out of the camera gradient), the
antialiased mode, filter_3d, capacity frames and sh_gradient="factored".  `dL_dmean2D_abs` stays the colour, depth and alpha terms'
alone.  Without the three keywords the call is exactly the one above.  (These four names are accepted by name through the
signature's catch-all `**rendered_stage`, checked against normal_render.STAGE_KEYWORDS; any other name is a TypeError.)

`dL_dmedian_depth=g, median_contributor=contrib` (include/gsr_median_depth.h; both or neither) add the gradient of
sum_p g[p] med[p], med and contrib the two results of median_depth.render_median_depth().  The median is piecewise constant in
everything but the chosen Gaussian's inverse depth, so the stage -- the last of the stages between the two halves, after the
distortion and normal stages -- ADDS g[p] into column 11 of the accumulator record of the Gaussian pixel p chose and touches nothing
else; the AUX per-Gaussian half carries it on to the means, and the result carries `dL_dinv_depths`.  `dL_dmedian_depth` alone is
legal (dL_dpixels=None).  A frame that does not carry the forward's records needs geom_buffer["depths"], as for the distortion term.
It composes with camera_grad, the antialiased mode, filter_3d, capacity frames and sh_gradient="factored"; `dL_dmean2D_abs` stays
the colour, depth and alpha terms' alone.  Without the two keywords the call is exactly the one above.

`dL_dplane_depth=g, plane_slopes=s, plane_depth_image=pd` (include/gsr_plane_depth.h; all three or none, and with them
`gaussian_normals=n`, the normals s = plane_depth.plane_slopes(n, ...) was made from) add the gradient of sum_p g[p] pd[p],
pd = plane_depth.render_plane_depth(s, ...) the blended ray-plane intersection inverse depth.  The stage runs between the two halves,
after the distortion and normal stages and before the median one: it ADDS its screen-space gradients into columns 3-4, 6, 7, 9 and 10
of the accumulator records -- never column 11, which stays the centre-depth terms' alone -- and writes `dL_dplane_moments`, an (N, 3)
buffer (sum w g, sum w g (p.x - x_k), sum w g (p.y - y_k)) that the result carries, with `dL_dinv_depths`.  After the per-Gaussian half
gsr_plane_slopes_backward turns the moments into the means' share, ADDED to dL_dmean3D, and dL/d(normals), which
gsr_gaussian_normals_backward carries on to dL_drot (a second call of it when the normal image's stage is present too: it adds), from
the scales (raw under filter_3d, as for the normals), rotations, means and viewmatrix AS THE CALLER PASSED THEM;
`plane_param_grad=False` skips both kernels, for callers who want only the moments.  `gaussian_normals` alone with these three keywords
belongs to this stage; with `dL_dnormal_image` and `normal_image` as well it serves both.  `dL_dplane_depth` alone is legal
(dL_dpixels=None).  A frame that does not carry the forward's records needs geom_buffer["depths"], as for the distortion term.  It
composes with camera_grad (the screen-space columns only), the antialiased mode, filter_3d, capacity frames and
sh_gradient="factored"; `dL_dmean2D_abs` stays the colour, depth and alpha terms' alone.  Without the three keywords the call is
exactly the one above.

The four stages between the two halves are described once each, in the order they run, in the table STAGES below.
"""
import ctypes as C
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import _frame, _host, _lib
from . import dist as _dist
from . import distortion as _distortion
from . import filter3d as _filter3d
from . import forward as _forward
from . import median_depth as _median_depth
from . import normal_render as _normal_render
from . import plane_depth as _plane_depth

_ZERO = {}


def _zeros_cov3d(n, dev):
    """The reference returns an all-zero dL_dcov3D (backward.py:1119 is allocated, never filled).  Here it is a real, dense
    (N, 6) zero tensor (`.view(-1)`, `.numpy()`, strides as the reference's array) that is cleared ONCE per (N, device) and
    then SHARED by every later call with that N: it is meant to be read.  A caller that writes into it changes what later
    calls return; `dL_dcov3D.clone()` gives a private copy."""
    z = _ZERO.get(dev.index)               # one entry per device, replaced when that device's N changes (a trainer's N changes
    if z is None or z.shape[0] != n:       # only at densification; a process that alternates two GPUs keeps both)
        z = _ZERO[dev.index] = torch.zeros((n, 6), dtype=torch.float32, device=dev)
    return z


def _aa_scale_of(conic_opacity, opacity, antialiased):
    """The antialiased forward's tag on its conic_opacity view (forward.py), or an error: an antialiased frame and a classic one
    are never taken for each other.  Returns the tag (rho, ..., the forward's device copy of a host opacity or None) or None."""
    tag = getattr(conic_opacity, "_gsr_aa_scale", None)
    if not antialiased:
        if tag is not None:
            raise ValueError("this frame was rendered with rasterize_mode='antialiased': pass the same mode to backward()")
        return None
    if tag is None:
        raise ValueError("backward(rasterize_mode='antialiased') needs the conic_opacity view of a frame rendered with "
                         "render_gaussians(rasterize_mode='antialiased'), not a copy of it and not a classic frame")
    _, op_ref, op_version, rec_version, _ = tag
    if conic_opacity._version != rec_version:
        raise ValueError("backward(rasterize_mode='antialiased'): the forward's records were written in place after the render")
    if op_ref is not None and not _host.unwritten((op_ref, op_version), opacity):
        raise ValueError("backward(rasterize_mode='antialiased'): `opacity` is not the tensor this frame was rendered from, or was "
                         "written in place since")
    return tag


def _get(buf, key):
    if buf is None:
        raise NameError(f"backward() needs the forward buffer holding '{key}' (the reference fails the same way, "
                        "backward.py:1084-1090)")
    return buf.get(key)


def _frame_state(given, dev, N, D, need, campos, degree, scale_modifier):
    """Which of the forward's state this call may use (forward.py hangs it on the frame's tensors as tags): each piece only while
    every tensor it was derived from, or is read against, is the forward's own and unwritten (_host.unwritten) -- identity, not
    equality -- and its plain conditions hold.  `given`: the caller's arrays as passed, by keyword.  Sets the five
    `backward.last_call_*` flags (for tests and debugging)."""
    unwritten = _host.unwritten
    s = SimpleNamespace(records=None, masks=None, order=None, sh_dir=None, recompute=False, cleared=None, D_bin=D)
    # the blend records (means2D / conic_opacity / rgb are columns of one (N, 16) tensor) stand in for the three arrays: no
    # re-pack, no packed copies of the views
    tag = getattr(given["means2D"], "_gsr_records", None)
    if tag is not None:
        rec, stamps = tag
        if all(unwritten(stamps[k], given[k]) for k in stamps) and rec.device == dev and rec.shape[0] == N:
            s.records = rec
    # the per-entry block masks (and the block order derived from them) are conservative only for THAT forward's records and
    # written only up to each tile's saturation batch: a caller who mixes in perturbed means2D / conic_opacity or another run's
    # ranges / n_contrib gets the self-contained block test instead
    point_list = given["point_list"]
    tag = getattr(point_list, "_gsr_block_masks", None)
    if tag is not None:
        m, stamps, order = tag
        if (all(unwritten(stamps[k], given[k]) for k in stamps) and isinstance(m, torch.Tensor) and m.dtype == torch.uint8
                and m.device == dev and m.numel() == D and m.is_contiguous()):
            s.masks, s.order = m, order
    # the d(colour)/d(direction) sums (GsrGeom.sh_dir_grad): geom_backward_kernel then reads 36 bytes per Gaussian instead of the
    # 192 bytes of coefficients
    tag = getattr(given["clamped"], "_gsr_sh_dir", None)
    if tag is not None:
        d, sh_stamp, means_stamp, campos_f, degree_f = tag
        if (unwritten(sh_stamp, given["shs"]) and unwritten(means_stamp, given["means3D"]) and degree_f == int(degree)
                and d.device == dev and campos_f == campos):
            s.sh_dir = d
    # Sigma3D is recomputed inside the kernel instead of read back (24 bytes per Gaussian; gsr.h GsrGeom.cov3D)
    cov3Ds = given["cov3Ds"]
    tag = getattr(cov3Ds, "_gsr_sigma_of", None)
    if tag is not None:
        cov_stamp, sc_stamp, rot_stamp, smod = tag
        s.recompute = (unwritten(cov_stamp, cov3Ds) and unwritten(sc_stamp, given["scales"]) and unwritten(rot_stamp, given["rotations"])
                       and smod == float(scale_modifier) and cov3Ds.device == dev and cov3Ds.shape[0] == N)
    # a capacity-mode point_list: K entries, the first D valid; GsrBinning.D is then the forward's shape hint
    # (include/gsr_capacity.h), so both sides pick the same blend block shape
    tag = getattr(point_list, "_gsr_capacity", None)
    if tag is not None:
        s.D_bin = tag[1]
    # "the forward cleared a backward workspace's accumulators" -- and no backward has taken it yet (_outputs takes it)
    tag = getattr(point_list, "_gsr_cleared_ws", None)
    if tag is not None and tag[0] is not None and tag[1] == N and tag[0].device == dev and tag[0].numel() >= need:
        s.cleared = tag
    backward.last_call_used_forward_records = s.records is not None
    backward.last_call_used_forward_masks = s.masks is not None
    backward.last_call_used_forward_sh_dir = s.sh_dir is not None
    backward.last_call_recomputed_sigma3d = s.recompute
    backward.last_call_skipped_the_clear = s.cleared is not None
    return s


def _outputs(L, dev, N, need, sh_gradient, cleared):
    """What the call writes: the gradient arena with its five views, the view payload, the workspace (which belongs to THIS call:
    the forward's pre-cleared one, taken here, so that a second backward() on the same forward gets a fresh one, which the library
    clears itself) and the blend-stage gradients as views of its accumulator records."""
    f32 = torch.float32
    factored = sh_gradient == "factored"
    o = _dist.arena_offsets(N, small=factored)     # every segment starts on a multiple of 4 floats (16-byte vector stores)
    arena = torch.empty(o[-1], dtype=f32, device=dev)
    if N % 4:                                      # the <= 3 padding floats behind a segment: defined (zero), never garbage
        for k, sz in enumerate([3 * N, 3 * N, 4 * N, N][:len(o) - 2]):
            arena[o[k] + sz:o[k + 1]].zero_()
    # the payload is its own allocation (aligned for the collective); "both": dense gradient AND the payload it factors into
    payload = torch.empty(N * 3 + 4, dtype=f32, device=dev) if sh_gradient != "dense" else None
    # always N*16 rows: the reference under-allocates for degree < 3 (quirk Q6)
    dL_dsh = None if factored else arena[o[4]:o[4] + 48 * N].view(N * 16, 3)
    if cleared is not None:
        ws, cleared[0] = cleared[0], None
    else:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    # dL_dcolor / dL_dmean2D / dL_dconic are columns 0-2 / 3-5 / 6-9 of the accumulator records the blend backward sums into
    # (gsr.h GsrGrads): strided views, so the per-Gaussian kernel does not write 40 bytes per Gaussian of copies
    off = int(L.gsr_backward_accumulators_offset(N))
    acc = ws[off:off + 64 * N].view(f32).view(N, 16)
    return SimpleNamespace(arena=arena, payload=payload, ws=ws, acc=acc, dL_dsh=dL_dsh,
                           dL_dmean3D=arena[o[0]:o[0] + 3 * N].view(N, 3), dL_dscale=arena[o[1]:o[1] + 3 * N].view(N, 3),
                           dL_drot=arena[o[2]:o[2] + 4 * N].view(N, 4), dL_dopacity=arena[o[3]:o[3] + N],
                           dL_dcolor=acc[:, 0:3], dL_dmean2D=acc[:, 3:6], dL_dconic=acc[:, 6:10])


def _normals_to_rotations(L, N, normals, scales, rot, means, cam, dnormals, out, dev, stream):
    """dL/d(normals) on to the quaternions (added): from the caller's scales (raw under filter_3d), rotations and means."""
    _lib.check(L.gsr_gaussian_normals_backward(N, _host.ptr(scales), _host.ptr(rot), _host.ptr(means), cam[0], _host.ptr(dnormals),
                                               _host.ptr(out.dL_drot), stream))


def _plane_moments_to_parameters(L, N, normals, scales, rot, means, cam, dmoments, out, dev, stream):
    """The plane stage's moments on to the means (added) and, through the normals, to the quaternions.  `cam`: the view matrix's
    floats, tan_fovx, tan_fovy, W, H."""
    dplane_n = torch.empty((N, 3), dtype=torch.float32, device=dev)
    _lib.check(L.gsr_plane_slopes_backward(N, _host.ptr(normals), _host.ptr(scales), _host.ptr(means), *cam, _host.ptr(dmoments),
                                           _host.ptr(out.dL_dmean3D), _host.ptr(dplane_n), stream))
    _normals_to_rotations(L, N, normals, scales, rot, means, cam, dplane_n, out, dev, stream)


# What _host.to_dev brings to the device for each stage: its keywords' values (in the order its check takes them) as the entry
# point's arrays after the frame, in the entry point's order.  `normals`: gaussian_normals, converted once for both stages it serves.
_F32, _I32, _to = torch.float32, torch.int32, _host.to_dev


def _distortion_inputs(dev, N, H, W, normals, dL_ddistortion, distortion_moments):
    return _to(dL_ddistortion, _F32, dev, (H, W)), _to(distortion_moments, _F32, dev, (H, W, 4))


def _normal_inputs(dev, N, H, W, normals, dL_dnormal_image, gaussian_normals, normal_image):
    return normals, _to(dL_dnormal_image, _F32, dev, (H, W, 3)), _to(normal_image, _F32, dev, (H, W, 3))


def _plane_inputs(dev, N, H, W, normals, dL_dplane_depth, plane_slopes, plane_depth_image, gaussian_normals):
    _plane_depth.check_slopes(plane_slopes, N)
    return _to(plane_slopes, _F32, dev, (N, 2)), _to(dL_dplane_depth, _F32, dev, (H, W)), _to(plane_depth_image, _F32, dev, (H, W))


def _median_inputs(dev, N, H, W, normals, dL_dmedian_depth, median_contributor):
    return _to(dL_dmedian_depth, _F32, dev, (H, W)), _to(median_contributor, _I32, dev, (H, W))


# A stage between the two halves, described once:
#   check, keywords   the all-or-none check of its keyword group, and the group in the order the check takes it
#   inputs            the function above: name, dtype and shape of every array it hands to the entry point
#   depths_reason     why a frame that does not carry the forward's records needs geom_buffer["depths"] for it (None: it does not; the
#                     entry point then takes the frame without 1 / depth, a GsrFeaturesFrame)
#   entry, result     the entry point -- (frame, *inputs, accumulator records[, result], stream) -- and the key of its (N, 3)
#                     per-Gaussian result, or None
#   param_grad, follow_up   after the per-Gaussian half, under this keyword
Stage = namedtuple("Stage", "name check keywords inputs depths_reason entry result param_grad follow_up")

# ... listed in the order they run
STAGES = (
    Stage("distortion", _distortion.check_gradient_pair, ("dL_ddistortion", "distortion_moments"), _distortion_inputs,
          "the distortion is a function of the Gaussians' inverse depths", "gsr_distortion_backward", None, None, None),
    Stage("normal", _normal_render.check_gradient_triple, ("dL_dnormal_image", "gaussian_normals", "normal_image"), _normal_inputs,
          None, "gsr_normal_render_backward", "dL_dgaussian_normals", "normal_param_grad", _normals_to_rotations),
    Stage("plane", _plane_depth.check_gradient_triple, ("dL_dplane_depth", "plane_slopes", "plane_depth_image", "gaussian_normals"), _plane_inputs,
          "the plane depth is a function of the Gaussians' inverse depths", "gsr_plane_depth_backward", "dL_dplane_moments", "plane_param_grad",
          _plane_moments_to_parameters),
    Stage("median", _median_depth.check_gradient_pair, ("dL_dmedian_depth", "median_contributor"), _median_inputs,
          "the per-Gaussian half carries dL/d(1/depth) on through the re-packed records", "gsr_median_depth_backward", None, None, None),
)
# the follow-ups add to dL_drot in this order, whatever the table's: the plane stage's, then the normal image's
FOLLOW_UP_ORDER = ("plane", "normal")


def _stages_present(dL_ddistortion, distortion_moments, dL_dnormal_image, gaussian_normals, normal_image, dL_dplane_depth, plane_slopes,
                    plane_depth_image, dL_dmedian_depth, median_contributor):
    """The stages a call's keywords ask for, in STAGES' order, each with its keywords' values: ((stage, values), ...).  The plain
    call: four checks and the empty tuple.  A group given in part is refused."""
    distortion, normal, plane, median = STAGES
    has_distortion = distortion.check(dL_ddistortion, distortion_moments)
    has_plane = plane.check(dL_dplane_depth, plane_slopes, plane_depth_image, gaussian_normals)
    # gaussian_normals alone with the three plane keywords belongs to the plane stage: the normal stage is then absent, not given in part
    has_normal = (not (has_plane and dL_dnormal_image is None and normal_image is None)
                  and normal.check(dL_dnormal_image, gaussian_normals, normal_image))
    has_median = median.check(dL_dmedian_depth, median_contributor)
    if not (has_distortion or has_normal or has_plane or has_median):
        return ()
    on = []
    if has_distortion:
        on.append((distortion, (dL_ddistortion, distortion_moments)))
    if has_normal:
        on.append((normal, (dL_dnormal_image, gaussian_normals, normal_image)))
    if has_plane:
        on.append((plane, (dL_dplane_depth, plane_slopes, plane_depth_image, gaussian_normals)))
    if has_median:
        on.append((median, (dL_dmedian_depth, median_contributor)))
    return tuple(on)


def _needs_depths(stage):
    return ValueError(f"backward({stage.keywords[0]}=...) on a frame that does not carry the forward's records needs "
                      f"geom_buffer['depths']: {stage.depths_reason}")


def _run_stages(L, stages, inputs, results, st, out, N, point_list, ranges, n_contrib, stream):
    """The stages' screen-space gradients (include/gsr_distortion.h, gsr_normal_render.h, gsr_plane_depth.h, gsr_median_depth.h), added
    into the accumulator records the blend half has just filled, and their per-Gaussian `results`.  The frame is read from the
    records that half blended with: the forward's own, or the re-packed ones at the head of the workspace (which carry 1 / depth:
    the caller passed the forward's depths).  On that second path the distortion's moments may have been formed from another
    reciprocal of the same depths (_frame.inv_depth_of divides in torch, the re-pack on the device): the two may differ in the last
    bit, so m - mu is then taken against a mean one ulp of m away from the forward's -- an error of the size of mu's own rounding,
    inside the bounds the re-packed case is tested at.  (The median stage's kernel reads the frame's lists and ranges only.)"""
    if N == 0:
        return
    if point_list.numel() == 0:
        for t in results.values():
            t.zero_()
        return
    rec = st.records if st.records is not None else out.ws[:64 * N].view(torch.float32).view(N, 16)
    frame = _frame.Frame.from_records(rec, point_list, ranges, n_contrib, st.masks)
    structs = {}                # at most two per call: with 1 / depth and without
    acc = out.acc.data_ptr()
    for (s, _), arrays in zip(stages, inputs):
        reads_depth = s.depths_reason is not None
        fs = structs.get(reads_depth)
        if fs is None:
            fs = structs[reads_depth] = C.byref(frame.struct(inv_depth=reads_depth))
        tail = (acc, stream) if s.result is None else (acc, _host.ptr(results[s.result]), stream)
        _lib.check(getattr(L, s.entry)(fs, *[_host.ptr(t) for t in arrays], *tail))


def _launch(L, scene, cam, geom, binning, img, pg, out, flags, aa_scale, aux, on_payload, camera_grad, stream, distortion=None):
    """One request, whatever the options (gsr_densify_stats.h): with no auxiliary gradient and no flag it runs gsr_backward's
    kernels.  One entry point per stage: `aa` is NULL in the classic mode, and the _aa exports are then the classic calls
    (csrc/api.hip).  `distortion`: None, or the stage or stages to run between the two halves (a callable).  Returns the camera gradient's
    36 floats, or None."""
    head = (C.byref(scene), C.byref(cam), C.byref(geom))
    ws, n_ws, aa = _host.ptr(out.ws), out.ws.numel(), _host.ptr(aa_scale)
    grads = _lib.GsrGrads(_host.ptr(out.dL_dmean3D), _host.ptr(out.dL_dscale), _host.ptr(out.dL_drot), _host.ptr(out.dL_dopacity),
                          _host.ptr(out.dL_dsh), None, None, None, _host.ptr(out.payload))
    if distortion is not None:
        # three parts: the blend half (with the view payload, which reads the colour columns only), the distortion stage, which adds
        # to columns 3-4, 6-7 and 9-11 of the accumulators, and the AUX per-Gaussian half, which carries column 11 on to the means
        _lib.check(L.gsr_backward_blend_flags(*head, C.byref(binning), C.byref(img), C.byref(pg), _host.ptr(out.payload), ws, n_ws, flags, stream))
        if on_payload is not None and out.payload is not None:
            on_payload(out.payload)
        distortion()
        grads.dL_drgb = None
        _lib.check(L.gsr_backward_geom_aa(*head, C.byref(grads), None, ws, n_ws, aa, stream))
    elif on_payload is not None and out.payload is not None:
        # two halves: the view payload is complete after the blend half, so the caller's hook can start its exchange
        # (an asynchronous all-gather) while the per-Gaussian half still runs
        _lib.check(L.gsr_backward_blend_flags(*head, C.byref(binning), C.byref(img), C.byref(pg), _host.ptr(out.payload), ws, n_ws, flags, stream))
        on_payload(out.payload)
        grads.dL_drgb = None
        if aa_scale is not None or aux:     # (the AUX per-Gaussian kernel: without an auxiliary gradient its one extra term is zero)
            _lib.check(L.gsr_backward_geom_aa(*head, C.byref(grads), None, ws, n_ws, aa, stream))
        else:                               # the classic split call's kernel
            _lib.check(L.gsr_backward_geom(*head, C.byref(grads), ws, n_ws, stream))
    else:
        _lib.check(L.gsr_backward_aa(*head, C.byref(binning), C.byref(img), C.byref(pg), C.byref(grads), None, ws, n_ws, flags, aa, stream))
    if not camera_grad:
        return None
    # after the backward, on the same stream and workspace: reads its accumulators, writes only its own output
    dcam = torch.empty(_lib.CAMERA_GRAD_FLOATS, dtype=torch.float32, device=out.ws.device)
    scratch = torch.empty(int(L.gsr_backward_camera_scratch_bytes(scene.N)), dtype=torch.uint8, device=out.ws.device)
    _lib.check(L.gsr_backward_camera_aa(*head, _host.ptr(dcam), ws, n_ws, _host.ptr(scratch), scratch.numel(), aa, stream))
    return dcam


def _result(out, N, dev, dcam, aux, absgrad):
    """The reference's nine keys, the arena and payload, and the keys the options add."""
    res = {
        "dL_dmean3D": out.dL_dmean3D, "dL_dcolor": out.dL_dcolor, "dL_dshs": out.dL_dsh, "dL_dopacity": out.dL_dopacity,
        "dL_dscale": out.dL_dscale, "dL_drot": out.dL_drot, "dL_dmean2D": out.dL_dmean2D, "dL_dconic": out.dL_dconic,
        "dL_dcov3D": _zeros_cov3d(N, dev),
        "_arena": out.arena,
        "_view_payload": out.payload,
    }
    if dcam is not None:
        res["dL_dviewmatrix"], res["dL_dprojmatrix"], res["dL_dcampos"] = dcam[0:16].view(4, 4), dcam[16:32].view(4, 4), dcam[32:35]
    if aux:
        res["dL_dinv_depths"] = out.acc[:, 11]      # GradRec slot 11 (gsr_gradrec_slot(9)): dL/d(1/depth) per Gaussian
    if absgrad:
        res["dL_dmean2D_abs"] = out.acc[:, 12:14]   # GradRec slots 12-13 (gsr_gradrec_slot(10), (11)): sums of |terms of dL_dmean2D|
    # for densify.DensifyStats.update: the workspace whose accumulators this call filled, unwritten since
    out.dL_dmean2D._gsr_backward_ws = (out.ws, out.ws._version, bool(absgrad), N)
    return res


def backward(background, means3D, dL_dpixels, opacity=None, shs=None, scales=None, rotations=None, scale_modifier=1.0,
             viewmatrix=None, projmatrix=None, tan_fovx=0.5, tan_fovy=0.5, image_height=256, image_width=256, campos=None,
             radii=None, means2D=None, conic_opacity=None, rgb=None, clamped=None, cov3Ds=None, geom_buffer=None,
             binning_buffer=None, img_buffer=None, degree=3, debug=False, *, sh_gradient="dense", on_payload=None,
             dL_ddepth_image=None, dL_dalpha_image=None, camera_grad=False, absgrad=False, rasterize_mode="classic", filter_3d=None,
             dL_ddistortion=None, distortion_moments=None, dL_dmedian_depth=None, median_contributor=None,
             dL_dplane_depth=None, plane_slopes=None, plane_depth_image=None, plane_param_grad=True, **rendered_stage):
    # The keywords of include/gsr_normal_render.h -- dL_dnormal_image, gaussian_normals, normal_image (None) and normal_param_grad (True)
    # -- are taken by name from `rendered_stage` (normal_render.stage_keywords), not listed above: tests/test_normals_abi.py holds that
    # the depth-normals stage of include/gsr_normals.h added no parameter whose name contains "normal" to this signature, by that
    # substring.  Any other name raises the TypeError an unknown keyword always gets.
    dL_dnormal_image, gaussian_normals, normal_image, normal_param_grad = _normal_render.stage_keywords(rendered_stage)
    antialiased = _lib.check_rasterize_mode(rasterize_mode)
    stages = _stages_present(dL_ddistortion, distortion_moments, dL_dnormal_image, gaussian_normals, normal_image, dL_dplane_depth, plane_slopes,
                             plane_depth_image, dL_dmedian_depth, median_contributor)
    frame_co = conic_opacity if conic_opacity is not None or geom_buffer is None else geom_buffer.get("conic_opacity")
    # (before anything touches the GPU: a frame rendered without the filter or with another one, raw tensors written since the render)
    if filter_3d is not None:
        _filter3d.check_filter_3d(filter_3d, means3D)
    filt = _filter3d.frame_tag(frame_co, filter_3d, scales, opacity)
    if filt is not None:
        # substitution, exactly: the backward below is that of the filtered scene the frame was rendered from (its own tensors, so
        # the antialiased tag and the Sigma3D recompute recognise them); the transpose of the map follows it, in place in the arena
        raw_scales, raw_opacity = scales, opacity
        scales, opacity = filt[0], filt[1]
    # (before anything touches the GPU: a frame of the other mode, a copy of the view, a write since the render)
    aa_tag = _aa_scale_of(frame_co, opacity, antialiased)
    if sh_gradient not in ("dense", "factored", "both"):
        raise ValueError("sh_gradient must be 'dense', 'factored' or 'both'")
    aux = dL_ddepth_image is not None or dL_dalpha_image is not None or stages != ()
    if dL_dpixels is None and not aux:
        raise ValueError("backward() needs dL_dpixels, dL_ddepth_image or dL_dalpha_image (or dL_ddistortion with distortion_moments, "
                         "dL_dnormal_image with gaussian_normals and normal_image, or dL_dmedian_depth with median_contributor, or "
                         "dL_dplane_depth with plane_slopes, plane_depth_image and gaussian_normals)")
    follow_ups = stages and [s for name in FOLLOW_UP_ORDER for s, _ in stages if s.name == name]      # (the plain call: () and nothing walked)
    view16 = _normal_render.view_floats(viewmatrix, "backward(dL_dnormal_image=...)") if follow_ups else None
    _forward._backward_seen = True     # from now on this process's forwards pre-clear the backward workspace (forward.PRECLEAR_BACKWARD)
    L = _lib.lib()
    dev = _host.device_of(means3D, dL_dpixels, shs, radii)
    H, W = int(image_height), int(image_width)
    f32, i32 = torch.float32, torch.int32
    opt = lambda x, shape: _host.to_dev(x, f32, dev, shape) if x is not None else None
    means = _host.to_dev(means3D, f32, dev, (-1, 3))
    N = means.shape[0]
    dpix, g_depth, g_alpha = opt(dL_dpixels, (H, W, 3)), opt(dL_ddepth_image, (H, W)), opt(dL_dalpha_image, (H, W))
    stage_in, stage_depths = None, None
    if stages:
        gn = opt(gaussian_normals, (N, 3))
        stage_in = [s.inputs(dev, N, H, W, gn, *values) for s, values in stages]
        for s, _ in stages:
            if s.depths_reason is not None:
                stage_depths = s        # the first stage that needs 1 / depth on a re-packed frame: the one a refusal names
                break
        param_grad = {"normal_param_grad": normal_param_grad, "plane_param_grad": plane_param_grad}
        follow_ups = [s for s in follow_ups if param_grad[s.param_grad] and N > 0]
        if dpix is None and g_depth is None and g_alpha is None:
            g_alpha = torch.zeros((H, W), dtype=f32, device=dev)   # the blend half wants one image gradient: a zero one clears and adds nothing
    sh = _host.to_dev(shs, f32, dev, (-1, 3))
    sc = _host.to_dev(scales, f32, dev, (-1, 3))
    rot = _host.to_dev(rotations, f32, dev, (-1, 4))
    op = _host.to_dev(opacity, f32, dev, (-1,)) if opacity is not None else means.new_zeros((N,))  # unused in the classic mode (quirk Q7)
    given = {"shs": shs, "means3D": means3D, "scales": scales, "rotations": rotations, "cov3Ds": cov3Ds,
             "ranges": _get(img_buffer, "ranges"), "final_Ts": _get(img_buffer, "final_Ts"), "n_contrib": _get(img_buffer, "n_contrib"),
             "point_list": _get(binning_buffer, "point_list")}      # reference backward.py:1084-1090
    if geom_buffer is not None:                               # reference backward.py:1092-1103
        radii = geom_buffer.get("radii") if radii is None else radii
        means2D = geom_buffer.get("means2D") if means2D is None else means2D
        conic_opacity = geom_buffer.get("conic_opacity") if conic_opacity is None else conic_opacity
        rgb = geom_buffer.get("rgb") if rgb is None else rgb
        clamped = geom_buffer.get("clamped_state") if clamped is None else clamped
    given.update(means2D=means2D, conic_opacity=conic_opacity, rgb=rgb, clamped=clamped)
    cam = _host.make_camera(viewmatrix, projmatrix, campos, background, tan_fovx, tan_fovy, W, H)
    D = given["point_list"].numel() if isinstance(given["point_list"], torch.Tensor) else int(np.size(given["point_list"]))
    need = int(L.gsr_backward_workspace_bytes(N, D, W, H))
    st = _frame_state(given, dev, N, D, need, tuple(cam.campos), degree, scale_modifier)

    radii = _host.to_dev(radii, i32, dev, (-1,))
    m2d = con = col = depths = None
    if st.records is None:      # (the reference re-reads the three arrays; so does this path -- packed copies if they are strided views)
        m2d = _host.to_dev(means2D, f32, dev, (-1, 2))
        con = _host.to_dev(conic_opacity, f32, dev, (-1, 4))
        col = _host.to_dev(rgb, f32, dev, (-1, 3))
        if (g_depth is not None or stage_depths is not None) and geom_buffer is not None:
            # the re-packed records carry 1/depth only from the forward's depths (gsr_aux_grads.h: without them, GSR_E_NULL)
            depths = opt(geom_buffer.get("depths"), (-1,))
        if stage_depths is not None and depths is None:
            raise _needs_depths(stage_depths)
    cl = _host.to_dev(clamped, f32, dev, (-1, 3))
    c3 = None if st.recompute else _host.to_dev(cov3Ds, f32, dev, (-1, 6))
    ranges = _host.to_dev(given["ranges"], i32, dev, (-1, 2))
    final_Ts = _host.to_dev(given["final_Ts"], f32, dev, (H, W))
    n_contrib = _host.to_dev(given["n_contrib"], i32, dev, (H, W))
    point_list = _host.to_dev(given["point_list"], i32, dev, (-1,))      # (D entries: counted above, for the frame state)
    aa_scale = None
    if antialiased:
        aa_scale, aa_op = aa_tag[0], aa_tag[4]
        if aa_scale.device != dev or aa_scale.shape[0] != N or op.shape[0] != N or (aa_op is not None and not torch.equal(aa_op, op)):
            raise ValueError("backward(rasterize_mode='antialiased'): `opacity` is not the opacity this frame was rendered from")
    scene = _lib.GsrScene(N, _host.ptr(means), _host.ptr(sc), _host.ptr(rot), _host.ptr(op), _host.ptr(sh), int(degree),
                          float(scale_modifier), 1)
    geom = _lib.GsrGeom(_host.ptr(radii), None, None, _host.ptr(m2d), _host.ptr(depths), _host.ptr(c3), _host.ptr(col), _host.ptr(con),
                        _host.ptr(cl), _host.ptr(st.records), _host.ptr(st.sh_dir))
    img = _lib.GsrImage(None, None, _host.ptr(final_Ts), _host.ptr(n_contrib))
    pg = _lib.GsrPixelGrads(_host.ptr(dpix), _host.ptr(g_depth), _host.ptr(g_alpha))
    cleared = st.cleared is not None
    with _host.on_device(dev):
        out = _outputs(L, dev, N, need, sh_gradient, st.cleared)
        binning = _lib.GsrBinning(st.D_bin, _host.ptr(point_list), _host.ptr(ranges), _host.ptr(st.masks), _host.ptr(st.order),
                                  _host.ptr(out.ws) if cleared else None, 1 if cleared else 0)
        stream = _host.raw_stream(dev)
        run_stages = stage_out = None
        if stages:
            # dL_dgaussian_normals: dL/d(gaussian_normals), what gsr_gaussian_normals_backward carries on to dL_drot; dL_dplane_moments:
            # what gsr_plane_slopes_backward carries on to dL_dmean3D and dL_drot
            stage_out = {s.result: torch.empty((N, 3), dtype=f32, device=dev) for s, _ in stages if s.result is not None}

            def run_stages():
                _run_stages(L, stages, stage_in, stage_out, st, out, N, point_list, ranges, n_contrib, stream)
        dcam = _launch(L, scene, cam, geom, binning, img, pg, out, _lib.BWD_ABSGRAD if absgrad else 0, aa_scale, aux, on_payload,
                       camera_grad, stream, run_stages)
        if follow_ups:
            nsc = sc if filt is None else _host.to_dev(raw_scales, f32, dev, (-1, 3))      # the raw scales under filter_3d
            view_cam = (view16[0], float(tan_fovx), float(tan_fovy), W, H)
            for s in follow_ups:
                s.follow_up(L, N, gn, nsc, rot, means, view_cam, stage_out[s.result], out, dev, stream)
        if filt is not None:
            _filter3d.filter_3d_backward(*_filter3d.raw_inputs(filt, raw_scales, raw_opacity, dev, N), filter_3d, out.dL_dscale, out.dL_dopacity)
    res = _result(out, N, dev, dcam, aux, absgrad)
    if stage_out:
        _host.written_in_place(*stage_out.values())
        res.update(stage_out)
    return res


def backward_view(params, camera, background, buffers, dL_dpixels, **kw):
    """backward() of a frame forward.render_view() drew: `buffers` is the dict it returned, regrouped here into the reference's
    arguments (points_xy_image -> means2D, colors -> rgb, clamped_state -> clamped, binning_buffer, img_buffer) -- the key names
    of three dicts, nothing else; the tensors go through as they are.  **kw: sh_gradient, camera_grad, absgrad, dL_ddepth_image,
    dL_dalpha_image, geom_buffer, rasterize_mode, filter_3d, dL_ddistortion with distortion_moments (a frame whose records were
    written since the render is re-packed from buffers["depths"], handed on here as geom_buffer), dL_dnormal_image with
    gaussian_normals and normal_image, normal_param_grad, dL_dmedian_depth with median_contributor (re-packed like the distortion term),
    dL_dplane_depth with plane_slopes, plane_depth_image and gaussian_normals (re-packed likewise), plane_param_grad."""
    get = kw.get
    stages = _stages_present(get("dL_ddistortion"), get("distortion_moments"), get("dL_dnormal_image"), get("gaussian_normals"), get("normal_image"),
                             get("dL_dplane_depth"), get("plane_slopes"), get("plane_depth_image"), get("dL_dmedian_depth"), get("median_contributor"))
    if any(s.depths_reason is not None for s, _ in stages) and "geom_buffer" not in kw and "depths" in buffers:
        kw["geom_buffer"] = {"depths": buffers["depths"]}
    return backward(background=background, means3D=params["positions"], dL_dpixels=dL_dpixels, opacity=params["opacities"],
                    shs=params["shs"], scales=params["scales"], rotations=params["rotations"], viewmatrix=camera["world_to_camera"],
                    projmatrix=camera["full_proj_matrix"], tan_fovx=camera["tan_fovx"], tan_fovy=camera["tan_fovy"],
                    image_height=camera["height"], image_width=camera["width"], campos=camera["camera_center"], radii=buffers["radii"],
                    means2D=buffers["points_xy_image"], conic_opacity=buffers["conic_opacity"], rgb=buffers["colors"],
                    cov3Ds=buffers["cov3Ds"], clamped=buffers["clamped_state"], binning_buffer={"point_list": buffers["point_list"]},
                    img_buffer={"ranges": buffers["ranges"], "final_Ts": buffers["final_Ts"], "n_contrib": buffers["n_contrib"]}, **kw)
