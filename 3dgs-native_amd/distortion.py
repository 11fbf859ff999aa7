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
from . import _frame, _host

inv_depth_of = _frame.inv_depth_of      # (it lives in _frame.py; still importable under its old name)


def render_distortion(buffers, image_height, image_width, out=None, use_block_masks=True):
    """(dist, moments): (H, W) float32 Dist(p) and (H, W, 4) float32 (A, mu, S, 0), the running sums the backward needs.  `out`: a
    caller-owned (dist, moments) pair to write into (every element is written).  use_block_masks=False walks without the forward's
    block masks (the same bits either way)."""
    fr = _frame.Frame.from_buffers(buffers, image_height, image_width, use_block_masks, inv_depth=True)
    dist, moments = fr.outputs(out, [(fr.H, fr.W), (fr.H, fr.W, 4)], pair="(dist, moments)")
    if fr.N == 0:
        return dist.zero_(), moments.zero_()
    fr.launch("gsr_distortion_forward", _host.ptr(dist), _host.ptr(moments), written=(dist, moments))
    return dist, moments


def check_gradient_pair(dL_ddistortion, distortion_moments):
    """backward()'s two keywords: both or neither."""
    if (dL_ddistortion is None) != (distortion_moments is None):
        raise ValueError("backward() needs dL_ddistortion and distortion_moments together: the moments are render_distortion()'s second result")
    return dL_ddistortion is not None
