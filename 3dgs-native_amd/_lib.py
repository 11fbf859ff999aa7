"""
ctypes binding of libgsr_hip.so (include/gsr.h).  The library is the only compute path: if it is
missing this module raises -- there is no Python, torch or CPU fallback behind it.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_LIB", os.path.join(_HERE, "libgsr_hip.so"))   # GSR_LIB: A/B runs of two builds on one box

MAX_RENDERED = 1 << 30      # GSR_MAX_RENDERED
GSR_OK, GSR_E_NULL, GSR_E_DIMS, GSR_E_OVERFLOW, GSR_E_WORKSPACE, GSR_E_HIP, GSR_E_CAPACITY, GSR_E_ALIGN = 0, -1, -2, -3, -4, -5, -6, -7

vp = C.c_void_p


class GsrScene(C.Structure):
    _fields_ = [("N", C.c_int64), ("means", vp), ("scales", vp), ("rotations", vp), ("opacity", vp), ("sh", vp),
                ("sh_degree", C.c_int32), ("scale_modifier", C.c_float), ("clamped", C.c_int32)]


class GsrCamera(C.Structure):
    _fields_ = [("view", C.c_float * 16), ("proj", C.c_float * 16), ("campos", C.c_float * 3), ("bg", C.c_float * 3),
                ("tan_fovx", C.c_float), ("tan_fovy", C.c_float), ("focal_x", C.c_float), ("focal_y", C.c_float),
                ("W", C.c_int32), ("H", C.c_int32)]


class GsrGeom(C.Structure):
    _fields_ = [("radii", vp), ("tiles_touched", vp), ("point_offsets", vp), ("xy", vp), ("depths", vp), ("cov3D", vp),
                ("rgb", vp), ("conic_opacity", vp), ("clamped_state", vp), ("blend_records", vp), ("sh_dir_grad", vp)]


class GsrBinning(C.Structure):
    _fields_ = [("D", C.c_int64), ("point_list", vp), ("ranges", vp), ("block_masks", vp), ("block_order", vp), ("backward_ws", vp),
                ("backward_ws_cleared", C.c_int32)]


class GsrImage(C.Structure):
    _fields_ = [("image", vp), ("inv_depth", vp), ("final_T", vp), ("n_contrib", vp)]


class GsrGrads(C.Structure):
    _fields_ = [("dL_dmean3D", vp), ("dL_dscale", vp), ("dL_drot", vp), ("dL_dopacity", vp), ("dL_dshs", vp),
                ("dL_dcolor", vp), ("dL_dmean2D", vp), ("dL_dconic", vp), ("dL_drgb", vp)]


class GsrAdamGroup(C.Structure):
    _fields_ = [("param", vp), ("grad", vp), ("m", vp), ("v", vp), ("lr", C.c_float)]


class GsrAdam(C.Structure):
    _fields_ = [("N", C.c_int64), ("pos", GsrAdamGroup), ("scale", GsrAdamGroup), ("rot", GsrAdamGroup),
                ("opacity", GsrAdamGroup), ("sh", GsrAdamGroup), ("beta1", C.c_float), ("beta2", C.c_float),
                ("epsilon", C.c_float), ("iteration", C.c_int32)]


class GsrParams(C.Structure):
    _fields_ = [("N", C.c_int64), ("positions", vp), ("scales", vp), ("rotations", vp), ("opacities", vp), ("shs", vp)]


MARK_CLONE, MARK_SPLIT = 0, 1

EXPORTS = {
    "gsr_abi_version": (C.c_int, []),
    "gsr_strerror": (C.c_char_p, [C.c_int]),
    "gsr_build_flags": (C.c_int, []),
    "gsr_geom_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_binning_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "gsr_backward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "gsr_backward_accumulators_offset": (C.c_size_t, [C.c_int64]),
    "gsr_block_order_ints": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_forward_count": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), vp, C.c_size_t,
                                    C.POINTER(C.c_int64), vp]),
    "gsr_forward_render": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrBinning),
                                     C.POINTER(GsrImage), vp, C.c_size_t, vp, C.c_size_t, vp]),
    "gsr_backward": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrBinning),
                               C.POINTER(GsrImage), vp, C.POINTER(GsrGrads), vp, C.c_size_t, vp]),
    "gsr_backward_blend": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrBinning),
                                     C.POINTER(GsrImage), vp, vp, vp, C.c_size_t, vp]),
    "gsr_backward_geom": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrGrads), vp, C.c_size_t, vp]),
    "gsr_l1_loss_grad": (C.c_int, [vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_float, vp]),
    "gsr_ssim": (C.c_int, [vp, vp, vp, C.c_int32, C.c_int32, vp]),
    "gsr_depth_loss": (C.c_int, [vp, vp, vp, vp, C.c_int32, C.c_int32, vp]),
    "gsr_adam_update": (C.c_int, [C.POINTER(GsrAdam), vp]),
    "gsr_adam_update_views": (C.c_int, [C.POINTER(GsrAdam), C.c_int32, C.c_int32, C.POINTER(vp), C.c_float, vp]),
    "gsr_sh_grad_from_views": (C.c_int, [C.c_int64, vp, C.c_int32, C.c_int32, C.POINTER(vp), C.c_float, vp, vp]),
    "gsr_densify_mark": (C.c_int, [C.POINTER(GsrParams), vp, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int, vp, vp]),
    "gsr_prune_mark": (C.c_int, [C.POINTER(GsrParams), C.c_float, vp, vp]),
    "gsr_split_removal_mask": (C.c_int, [C.c_int64, C.c_int64, vp, vp, vp]),
    "gsr_mask_scan_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_mask_scan": (C.c_int, [C.c_int64, vp, vp, C.POINTER(C.c_int32), vp, C.c_size_t, vp]),
    "gsr_clone_gaussians": (C.c_int, [C.POINTER(GsrParams), vp, vp, C.c_float, C.POINTER(GsrParams), vp]),
    "gsr_split_gaussians": (C.c_int, [C.POINTER(GsrParams), vp, vp, C.c_int32, C.c_float, C.POINTER(GsrParams), vp]),
    "gsr_compact_gaussians": (C.c_int, [C.POINTER(GsrParams), vp, vp, C.POINTER(GsrParams), vp]),
    "gsr_init_gaussians": (C.c_int, [C.POINTER(GsrParams), C.c_float, vp]),
    "gsr_reset_opacities": (C.c_int, [C.c_int64, C.c_float, vp, vp]),
    "gsr_stage_timing": (C.c_int, [C.c_int, C.c_int]),
    "gsr_stage_sampling": (C.c_int, [C.c_int]),
    "gsr_stage_times": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_int)]),
}

# include/gsr_capacity.h: the capacity-mode forward (its own header, so its own table)
CAPACITY_EXPORTS = {
    "gsr_forward_capacity": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrBinning),
                                       C.POINTER(GsrImage), vp, C.c_size_t, vp, C.c_size_t, C.c_int64, vp]),
}

# include/gsr_loss.h: the L1 + D-SSIM training loss with its pixel gradient (its own header, so its own table)
LOSS_EXPORTS = {
    "gsr_dssim_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_l1_dssim_loss_grad": (C.c_int, [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_float, C.c_int32, vp, C.c_size_t, vp]),
}
SSIM_WINDOWS = {"reference": 0, "gaussian": 1}   # GSR_SSIM_WINDOW_REFERENCE / GSR_SSIM_WINDOW_GAUSSIAN


class GsrPixelGrads(C.Structure):
    _fields_ = [("dL_dpixels", vp), ("dL_dinv_depth", vp), ("dL_dalpha", vp)]


# include/gsr_aux_grads.h: the backward through the inverse-depth and alpha images, and their losses (its own header, so its own table)
AUX_EXPORTS = {
    "gsr_backward_aux": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrBinning),
                                   C.POINTER(GsrImage), C.POINTER(GsrPixelGrads), C.POINTER(GsrGrads), vp, vp, C.c_size_t, vp]),
    "gsr_backward_blend_aux": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrBinning),
                                         C.POINTER(GsrImage), C.POINTER(GsrPixelGrads), vp, vp, C.c_size_t, vp]),
    "gsr_backward_geom_aux": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrGrads), vp, vp,
                                        C.c_size_t, vp]),
    "gsr_depth_loss_grad": (C.c_int, [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_float, vp]),
    "gsr_alpha_loss_grad": (C.c_int, [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_float, vp]),
}

# include/gsr_camera_grads.h: dL/d(view, proj, campos) after a backward (its own header, so its own table)
CAMERA_EXPORTS = {
    "gsr_backward_camera_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_backward_camera": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), vp, vp, C.c_size_t, vp, C.c_size_t,
                                      vp]),
}
CAMERA_GRAD_FLOATS = 36     # GSR_CAMERA_GRAD_FLOATS: view 0-15 | proj 16-31 | campos 32-34 | 0



class GsrDensifyStats(C.Structure):
    _fields_ = [("N", C.c_int64), ("grad_accum", vp), ("vis_count", vp), ("max_radii", vp)]


# include/gsr_densify_stats.h: screen-space densification statistics and the absolute-gradient backward (its own header, so its own table)
DENSIFY_STATS_EXPORTS = {
    "gsr_backward_flags": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrBinning),
                                     C.POINTER(GsrImage), C.POINTER(GsrPixelGrads), C.POINTER(GsrGrads), vp, vp, C.c_size_t, C.c_uint32, vp]),
    "gsr_backward_blend_flags": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrBinning),
                                           C.POINTER(GsrImage), C.POINTER(GsrPixelGrads), vp, vp, C.c_size_t, C.c_uint32, vp]),
    "gsr_densify_stats_update": (C.c_int, [C.POINTER(GsrDensifyStats), vp, vp, C.c_size_t, C.c_int32, vp]),
    "gsr_densify_mark_stats": (C.c_int, [C.POINTER(GsrParams), C.POINTER(GsrDensifyStats), C.c_float, C.c_float, C.c_float, C.c_int, vp, vp]),
    "gsr_prune_mark_stats": (C.c_int, [C.POINTER(GsrParams), C.POINTER(GsrDensifyStats), C.c_float, C.c_float, C.c_float, vp, vp]),
}
BWD_ABSGRAD = 1             # GSR_BWD_ABSGRAD

# include/gsr_antialias.h: the antialiased mode (opacity compensation of the screen-space blur), selected by one more argument,
# `aa_scale` (its own header, so its own table)
ANTIALIAS_EXPORTS = {
    "gsr_forward_count_aa": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), vp, C.c_size_t,
                                       C.POINTER(C.c_int64), vp, vp]),
    "gsr_forward_capacity_aa": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrBinning),
                                          C.POINTER(GsrImage), vp, C.c_size_t, vp, C.c_size_t, C.c_int64, vp, vp]),
    "gsr_backward_aa": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrBinning),
                                  C.POINTER(GsrImage), C.POINTER(GsrPixelGrads), C.POINTER(GsrGrads), vp, vp, C.c_size_t, C.c_uint32, vp, vp]),
    "gsr_backward_geom_aa": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), C.POINTER(GsrGrads), vp, vp,
                                       C.c_size_t, vp, vp]),
    "gsr_backward_camera_aa": (C.c_int, [C.POINTER(GsrScene), C.POINTER(GsrCamera), C.POINTER(GsrGeom), vp, vp, C.c_size_t, vp, C.c_size_t,
                                         vp, vp]),
}
RASTERIZE_MODES = ("classic", "antialiased")


class GsrFilterView(C.Structure):
    _fields_ = [("view", C.c_float * 16), ("focal", C.c_float), ("W", C.c_int32), ("H", C.c_int32), ("pad", C.c_int32)]   # 80 bytes


# include/gsr_filter3d.h: the 3D smoothing filter (Mip-Splatting): sampling rates from the training views, the map on
# (scales, opacity) and its transpose (its own header, so its own table)
FILTER3D_EXPORTS = {
    "gsr_filter3d_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_filter3d_from_views": (C.c_int, [C.c_int64, vp, C.c_int32, vp, C.c_float, vp, vp, C.c_size_t, vp]),
    "gsr_filter3d_apply": (C.c_int, [C.c_int64, vp, vp, vp, vp, vp, vp]),
    "gsr_filter3d_backward": (C.c_int, [C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp]),
}
FILTER3D_VARIANCE = 0.2     # GSR_FILTER3D_VARIANCE

# include/gsr_exposure.h: per-view exposure compensation, c' = c A + b on the rendered image, its backward and the Adam step of
# one view's 12 numbers (its own header, so its own table)
EXPOSURE_EXPORTS = {
    "gsr_exposure_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_exposure_apply": (C.c_int, [vp, vp, vp, C.c_int32, C.c_int32, vp]),
    "gsr_exposure_backward": (C.c_int, [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, vp, C.c_size_t, vp]),
    "gsr_exposure_adam": (C.c_int, [vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, vp]),
}
EXPOSURE_FLOATS = 12            # GSR_EXPOSURE_FLOATS
EXPOSURE_BLOCK_PIXELS = 1024    # GSR_EXPOSURE_BLOCK_PIXELS
EXPOSURE_MAX_BLOCKS = 1024      # GSR_EXPOSURE_MAX_BLOCKS
EXPOSURE_RECORD_BYTES = 64      # GSR_EXPOSURE_RECORD_BYTES

# include/gsr_weighted_loss.h: the colour loss under per-pixel weights (its own header, so its own table)
WEIGHTED_LOSS_EXPORTS = {
    "gsr_weight_total_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_weight_total": (C.c_int, [vp, C.c_int32, C.c_int32, vp, vp, C.c_size_t, vp]),
    "gsr_weighted_l1_loss_grad": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_float, vp, C.c_size_t, vp]),
    "gsr_weighted_dssim_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_weighted_l1_dssim_loss_grad": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_float, C.c_int32, vp, C.c_size_t, vp]),
}

# include/gsr_depth_corr.h: the Pearson-correlation depth loss, 1 - rho(rendered inverse depth, target), for depth priors known up to
# a scale and a shift per image (its own header, so its own table)
DEPTH_CORR_EXPORTS = {
    "gsr_depth_corr_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_depth_corr_loss_grad": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_float, vp, C.c_size_t, vp]),
}
DEPTH_CORR_FIT_FLOATS = 4           # GSR_DEPTH_CORR_FIT_FLOATS: (rho, s, b, M)
DEPTH_CORR_BLOCK_PIXELS = 1024      # GSR_DEPTH_CORR_BLOCK_PIXELS
DEPTH_CORR_MAX_BLOCKS = 1024        # GSR_DEPTH_CORR_MAX_BLOCKS
DEPTH_CORR_RECORD_BYTES = 64        # GSR_DEPTH_CORR_RECORD_BYTES
DEPTH_CORR_MIN_REL_VAR = 1e-12      # GSR_DEPTH_CORR_MIN_REL_VAR

# include/gsr_knn.h: exact 3-nearest-neighbour distances of a point cloud, the start of a run from SfM or random points (its own
# header, so its own table)
KNN_EXPORTS = {
    "gsr_knn_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_knn": (C.c_int, [C.c_int64, vp, vp, vp, vp, C.c_size_t, vp]),
}
KNN_K = 3                           # GSR_KNN_K
KNN_BLOCK_POINTS = 256              # GSR_KNN_BLOCK_POINTS
KNN_MAX_POINTS = 1 << 27            # GSR_KNN_MAX_POINTS

class GsrFeaturesFrame(C.Structure):
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("N", C.c_int64), ("D", C.c_int64), ("xy", vp), ("xy_stride", C.c_int64),
                ("conic_opacity", vp), ("conic_opacity_stride", C.c_int64), ("point_list", vp), ("ranges", vp), ("n_contrib", vp),
                ("block_masks", vp)]


# include/gsr_features.h: N-channel feature rendering over a frame's lists, and its gradient with respect to the features (its own
# header, so its own table)
FEATURES_EXPORTS = {
    "gsr_features_forward": (C.c_int, [C.POINTER(GsrFeaturesFrame), C.c_int32, vp, vp, vp]),
    "gsr_features_backward": (C.c_int, [C.POINTER(GsrFeaturesFrame), C.c_int32, vp, vp, vp]),
}
FEATURES_MAX_CHANNELS = 64          # GSR_FEATURES_MAX_CHANNELS
FEATURES_MAX_SIDE = 32768           # GSR_FEATURES_MAX_SIDE

class GsrDistortionFrame(C.Structure):
    _fields_ = GsrFeaturesFrame._fields_ + [("inv_depth", vp), ("inv_depth_stride", C.c_int64)]


# include/gsr_distortion.h: the depth-distortion regulariser over a frame's lists, and its gradient into the backward's
# accumulator records (its own header, so its own table)
DISTORTION_EXPORTS = {
    "gsr_distortion_forward": (C.c_int, [C.POINTER(GsrDistortionFrame), vp, vp, vp]),
    "gsr_distortion_backward": (C.c_int, [C.POINTER(GsrDistortionFrame), vp, vp, vp, vp]),
}

# include/gsr_median_depth.h: the median inverse depth over a frame's lists (the frame struct is gsr_distortion.h's), and its gradient
# into column 11 of the backward's accumulator records (its own header, so its own table)
MEDIAN_DEPTH_EXPORTS = {
    "gsr_median_depth_forward": (C.c_int, [C.POINTER(GsrDistortionFrame), vp, vp, vp]),
    "gsr_median_depth_backward": (C.c_int, [C.POINTER(GsrDistortionFrame), vp, vp, vp, vp]),
}

# include/gsr_plane_depth.h: the ray-plane intersection depth over a frame's lists (the frame struct is gsr_distortion.h's), the
# per-Gaussian slopes it blends, and the gradients of both (its own header, so its own table)
PLANE_DEPTH_EXPORTS = {
    "gsr_plane_slopes": (C.c_int, [C.c_int64, vp, vp, vp, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_int32, C.c_int32, vp, vp]),
    "gsr_plane_slopes_backward": (C.c_int, [C.c_int64, vp, vp, vp, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_int32, C.c_int32, vp, vp, vp, vp]),
    "gsr_plane_depth_forward": (C.c_int, [C.POINTER(GsrDistortionFrame), vp, vp, vp]),
    "gsr_plane_depth_backward": (C.c_int, [C.POINTER(GsrDistortionFrame), vp, vp, vp, vp, vp, vp]),
}
PLANE_DEPTH_MIN_COS = 0.1           # GSR_PLANE_DEPTH_MIN_COS (a float32 constant: 0.1f)
PLANE_DEPTH_MAX_FLATNESS = 0.5      # GSR_PLANE_DEPTH_MAX_FLATNESS
PLANE_DEPTH_NEAR = 0.2              # GSR_PLANE_DEPTH_NEAR (a float32 constant: 0.2f)
PLANE_DEPTH_MAX_RATIO = 4.0         # GSR_PLANE_DEPTH_MAX_RATIO

# include/gsr_plane_median.h: the ray-plane intersection depth under the median rule over a frame's lists (the frame struct is
# gsr_distortion.h's, the slopes gsr_plane_depth.h's), and its gradient into the plane moments (its own header, so its own table)
PLANE_MEDIAN_EXPORTS = {
    "gsr_pmed_forward": (C.c_int, [C.POINTER(GsrDistortionFrame), vp, vp, vp, vp]),
    "gsr_pmed_backward": (C.c_int, [C.POINTER(GsrDistortionFrame), vp, vp, vp, vp, vp]),
}

# include/gsr_normal_render.h: the Gaussians' own normals, their image over a frame's lists with its gradient into the backward's
# accumulator records, and the depth-normal consistency term (its own header, so its own table)
NORMAL_RENDER_EXPORTS = {
    "gsr_gaussian_normals": (C.c_int, [C.c_int64, vp, vp, vp, C.POINTER(C.c_float), vp, vp]),
    "gsr_gaussian_normals_backward": (C.c_int, [C.c_int64, vp, vp, vp, C.POINTER(C.c_float), vp, vp, vp]),
    "gsr_normal_render_forward": (C.c_int, [C.POINTER(GsrFeaturesFrame), vp, vp, vp]),
    "gsr_normal_render_backward": (C.c_int, [C.POINTER(GsrFeaturesFrame), vp, vp, vp, vp, vp, vp]),
    "gsr_normal_consistency_loss": (C.c_int, [vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_float, vp, vp, vp, vp, C.c_size_t, vp]),
}
NORMAL_RENDER_MIN_AXIS2 = 1e-24     # GSR_NORMAL_RENDER_MIN_AXIS2 (a float32 constant: 1e-24f)
NORMAL_RENDER_MIN_LENGTH = 1e-3     # GSR_NORMAL_RENDER_MIN_LENGTH (a float32 constant: 1e-3f)

# include/gsr_normals.h: surface normals from the rendered depth, their gradient back to the inverse-depth and alpha images, and the
# cosine loss against a normal prior (its own header, so its own table)
NORMALS_EXPORTS = {
    "gsr_normals_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_normals_from_depth": (C.c_int, [vp, vp, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_float, vp, vp, vp]),
    "gsr_normals_from_depth_backward": (C.c_int, [vp, vp, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_float, vp, vp, vp, vp, C.c_size_t, vp]),
    "gsr_normals_loss_grad": (C.c_int, [vp, vp, vp, C.POINTER(C.c_float), vp, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                        vp, vp, vp, vp, C.c_size_t, vp]),
}
NORMALS_MIN_NORM2 = 1e-12           # GSR_NORMALS_MIN_NORM2 (a float32 constant: 1e-12f)
NORMALS_ALPHA_MIN = 0.5             # GSR_NORMALS_ALPHA_MIN
NORMALS_TILE_W = 32                 # GSR_NORMALS_TILE_W
NORMALS_TILE_H = 8                  # GSR_NORMALS_TILE_H
NORMALS_MAX_BLOCKS = 2048           # GSR_NORMALS_MAX_BLOCKS
NORMALS_RECORD_BYTES = 16           # GSR_NORMALS_RECORD_BYTES
NORMALS_SUMS_FLOATS = 2             # GSR_NORMALS_SUMS_FLOATS: (loss_sum, weight_sum)

class GsrTsdfVolume(C.Structure):
    _fields_ = [("Gx", C.c_int32), ("Gy", C.c_int32), ("Gz", C.c_int32), ("voxel_size", C.c_float), ("origin", C.c_float * 3), ("pad", C.c_int32),
                ("tsdf", vp), ("weight", vp), ("color", vp)]


class GsrTsdfView(C.Structure):
    _fields_ = [("depth", vp), ("color", vp), ("view", C.c_float * 16), ("tan_fovx", C.c_float), ("tan_fovy", C.c_float), ("W", C.c_int32),
                ("H", C.c_int32), ("w_obs", C.c_float), ("pad", C.c_int32)]   # 104 bytes


# include/gsr_tsdf.h: TSDF fusion of depth images into a dense volume and marching-tetrahedra mesh extraction (its own header, so its
# own table)
TSDF_EXPORTS = {
    "gsr_mesh_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "gsr_tsdf_reset": (C.c_int, [C.POINTER(GsrTsdfVolume), vp]),
    "gsr_tsdf_integrate": (C.c_int, [C.POINTER(GsrTsdfVolume), C.c_int32, C.POINTER(GsrTsdfView), C.c_float, C.c_float, C.c_float, vp]),
    "gsr_tsdf_depth": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_float, vp, vp]),
    "gsr_mesh_count": (C.c_int, [C.POINTER(GsrTsdfVolume), C.c_float, vp, C.c_size_t, vp, vp]),
    "gsr_mesh_emit": (C.c_int, [C.POINTER(GsrTsdfVolume), C.c_float, vp, C.c_size_t, C.c_int64, vp, vp, vp, vp]),
}
TSDF_MAX_DIM = 2048                 # GSR_TSDF_MAX_DIM
TSDF_MAX_VOXELS = 1 << 31           # GSR_TSDF_MAX_VOXELS
TSDF_MAX_SIDE = 1 << 24             # GSR_TSDF_MAX_SIDE
TSDF_VIEWS_PER_LAUNCH = 16          # GSR_TSDF_VIEWS_PER_LAUNCH
MESH_GROUP_CELLS = 256              # GSR_MESH_GROUP_CELLS
MESH_SCAN_GROUPS = 1024             # GSR_MESH_SCAN_GROUPS
MESH_DIRECTIONS = 7                 # GSR_MESH_DIRECTIONS

# include/gsr_mesh_eval.h: points sampled on a triangle mesh by area and the exact nearest neighbour across two point sets, what the
# accuracy / completeness / F-score of an extracted mesh are made of (its own header, so its own table)
MESH_EVAL_EXPORTS = {
    "gsr_nearest_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gsr_nearest": (C.c_int, [C.c_int64, vp, C.c_int64, vp, C.c_float, vp, vp, vp, C.c_size_t, vp]),
    "gsr_surface_sample_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_surface_sample_count": (C.c_int, [C.c_int64, vp, C.c_float, C.c_uint32, vp, vp, C.c_size_t, vp]),
    "gsr_surface_sample_emit": (C.c_int, [C.c_int64, vp, vp, C.c_uint32, C.c_int64, vp, vp, vp]),
}
NEAREST_BLOCK_POINTS = 256                  # GSR_NEAREST_BLOCK_POINTS
NEAREST_MAX_POINTS = 1 << 27                # GSR_NEAREST_MAX_POINTS
SURFACE_SAMPLE_MAX_TRIANGLES = 1 << 27      # GSR_SURFACE_SAMPLE_MAX_TRIANGLES
SURFACE_SAMPLE_MAX_SAMPLES = 1 << 27        # GSR_SURFACE_SAMPLE_MAX_SAMPLES
SURFACE_SAMPLE_MAX_PER_TRIANGLE = 1 << 20   # GSR_SURFACE_SAMPLE_MAX_PER_TRIANGLE

# include/gsr_debug_layout.h: where the forward's tile-order tables lie inside the geom workspace, for tests and tools (its own
# header, so its own table)
DEBUG_LAYOUT_EXPORTS = {
    "gsr_fwd_order_tables_offset": (C.c_int, [C.c_int64, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
}
FWD_ORDER_MAX_TILES = 4096      # GSR_FWD_ORDER_MAX_TILES



def check_rasterize_mode(mode):
    """The `rasterize_mode` keyword of render_gaussians() and backward(): refused before the library is touched."""
    if mode not in RASTERIZE_MODES:
        raise ValueError(f"rasterize_mode must be 'classic' or 'antialiased' (got {mode!r})")
    return mode == "antialiased"

STAGES = ["preprocess", "scan", "depth_sort", "host_gap", "depth_scan", "expand", "tile_sort", "ranges", "blend_fwd",
          "bwd_prep", "blend_bwd", "geom_bwd"]

_lib = None


def lib():
    """Load libgsr_hip.so once.  Raises if it has not been built (`__graft_entry__.build()`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950).  There is no fallback path.")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in (list(EXPORTS.items()) + list(CAPACITY_EXPORTS.items()) + list(LOSS_EXPORTS.items())
                                  + list(AUX_EXPORTS.items()) + list(CAMERA_EXPORTS.items())
                                  + list(DENSIFY_STATS_EXPORTS.items()) + list(ANTIALIAS_EXPORTS.items())
                                  + list(FILTER3D_EXPORTS.items()) + list(EXPOSURE_EXPORTS.items())
                                  + list(DEBUG_LAYOUT_EXPORTS.items()) + list(WEIGHTED_LOSS_EXPORTS.items())
                                  + list(DEPTH_CORR_EXPORTS.items()) + list(KNN_EXPORTS.items())
                                  + list(FEATURES_EXPORTS.items()) + list(NORMALS_EXPORTS.items())
                                  + list(TSDF_EXPORTS.items()) + list(DISTORTION_EXPORTS.items())
                                  + list(NORMAL_RENDER_EXPORTS.items()) + list(MESH_EVAL_EXPORTS.items())
                                  + list(MEDIAN_DEPTH_EXPORTS.items()) + list(PLANE_DEPTH_EXPORTS.items())
                                  + list(PLANE_MEDIAN_EXPORTS.items())):
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
        if h.gsr_abi_version() != 7:
            raise RuntimeError("libgsr_hip.so ABI version mismatch")
        _lib = h
    return _lib


def build_hash():
    """First 16 hex digits of the SHA-256 of the loaded library file: the key under which profiles/ stores per-build counters."""
    import hashlib
    with open(LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def strerror(code):
    return lib().gsr_strerror(code).decode()


def check(code):
    """Map a GSR_E_* return code to the exception the reference would raise."""
    if code == GSR_OK:
        return
    if code == GSR_E_OVERFLOW:   # reference forward.py:765-767 raises ValueError
        raise ValueError("Number of rendered points exceeds the maximum supported (2^30).")
    raise RuntimeError(f"libgsr_hip: {strerror(code)} (code {code})")


def stage_timing(enable, max_steps=256, every=1):
    """Record per-stage HIP events on one forward/backward pair in `every` (event records are not free).  every = 0 creates the
    events but records nothing until stage_sampling(k >= 1): a benchmark allocates them before its warm-up and switches them on
    only for steps it does not time."""
    check(lib().gsr_stage_timing(1 if enable else 0, int(max_steps)))
    if enable:
        check(lib().gsr_stage_sampling(int(every)))


def stage_sampling(every):
    """0 = pause the recording (events stay allocated), k >= 1 = record one forward/backward pair in k."""
    check(lib().gsr_stage_sampling(int(every)))


def stage_times():
    """Average ms per stage over the steps recorded since stage_timing(True); synchronise first."""
    arr = (C.c_float * len(STAGES))()
    n = C.c_int(0)
    check(lib().gsr_stage_times(arr, C.byref(n)))
    return {k: float(arr[i]) for i, k in enumerate(STAGES)}, n.value
