"""
The median inverse depth over the lists of a rendered frame (include/gsr_median_depth.h) over the MI355X library: per pixel, the
inverse view depth of the Gaussian at which the transmittance falls through one half (2DGS's rule) -- the depth 2DGS, GOF, PGSR and
RaDe-GS fuse bounded scenes from, where the forward's depth image is the expected inverse depth sum w m.

    image, depth, buffers = render_gaussians(...)                        # any rasterize_mode, with or without filter_3d
    med, contrib = render_median_depth(buffers, H, W)                    # (H, W) float32 1 / depth and (H, W) int32 list position
    z = view_depth(med, buffers["final_Ts"])                             # (H, W) view depth, 0 where there is no surface: for TSDF fusion
    grads = backward(..., dL_dmedian_depth=g, median_contributor=contrib)   # g = dL/d(med), (H, W): into dL_dinv_depths and the means

The forward gives the same bits every call.  The median is piecewise constant in everything but the chosen Gaussian's inverse depth,
so its gradient is a scatter of g to that Gaussian, a stage of backward() between the blend half and the per-Gaussian half
(backward.py).  A capacity-mode frame is to be used only once rendered_count(buffers) has said that it did not overflow.  Everything
is enqueued on the current stream; nothing is read back.
"""
import torch

from . import _frame, _host, _lib


def render_median_depth(buffers, image_height, image_width, out=None, use_block_masks=True):
    """(median_inv_depth, median_contrib): (H, W) float32, the chosen Gaussian's 1 / depth bit for bit, and (H, W) int32, its 1-based
    position in the tile's list (n_contrib's convention; 0 and a value of 0 where no entry was applied).  `out`: a caller-owned pair
    to write into (every element is written).  use_block_masks=False walks without the forward's block masks (the same bits either
    way)."""
    fr = _frame.Frame.from_buffers(buffers, image_height, image_width, use_block_masks, inv_depth=True)
    med, contrib = fr.outputs(out, [(fr.H, fr.W), (fr.H, fr.W)], pair="(median_inv_depth, median_contrib)", dtypes=(torch.float32, torch.int32))
    if fr.N == 0:
        return med.zero_(), contrib.zero_()
    fr.launch("gsr_median_depth_forward", _host.ptr(med), _host.ptr(contrib), written=(med, contrib))
    return med, contrib


def view_depth(median_inv_depth, final_Ts, alpha_min=_lib.NORMALS_ALPHA_MIN):
    """(H, W) view depth for TSDF fusion: 1 / med where med > 0 and the coverage 1 - final_Ts >= alpha_min, both finite, and 0
    elsewhere -- tsdf.depth_from_buffers' rule, on the median instead of the expected inverse depth over the coverage.  Plain torch:
    extraction is offline."""
    if not (torch.is_tensor(median_inv_depth) and torch.is_tensor(final_Ts) and median_inv_depth.dim() == 2
            and median_inv_depth.shape == final_Ts.shape and median_inv_depth.dtype == final_Ts.dtype == torch.float32
            and median_inv_depth.device == final_Ts.device):
        raise ValueError("median_inv_depth and final_Ts must be (H, W) float32 tensors of one shape on one device")
    alpha_min = float(alpha_min)
    if not 0.0 < alpha_min <= 1.0:
        raise ValueError("alpha_min must lie in (0, 1]")
    cover = 1.0 - final_Ts
    ok = torch.isfinite(median_inv_depth) & torch.isfinite(cover) & (median_inv_depth > 0) & (cover >= alpha_min)
    return torch.where(ok, 1.0 / torch.where(ok, median_inv_depth, torch.ones_like(median_inv_depth)), torch.zeros_like(median_inv_depth))


def check_gradient_pair(dL_dmedian_depth, median_contributor):
    """backward()'s two keywords: both or neither."""
    if (dL_dmedian_depth is None) != (median_contributor is None):
        raise ValueError("backward() needs dL_dmedian_depth and median_contributor together: the contributor image is "
                         "render_median_depth()'s second result")
    return dL_dmedian_depth is not None
