"""
N-channel feature rendering over the lists of a rendered frame (include/gsr_features.h) over the MI355X library: any per-Gaussian
quantity -- a normal, a segmentation logit, a distilled 2D feature, a statistic, an id as a palette colour -- as an image, blended
with the weights of a frame render_gaussians() has already drawn, and the gradient of that image with respect to the features.

    image, depth, buffers = render_gaussians(...)                        # any rasterize_mode, with or without filter_3d
    out = render_features(F, buffers, H, W)                              # (H, W, C) float32; F is (N, C), 1 <= C <= 64
    dF = render_features_backward(G, buffers, H, W)                      # (N, C): the transposed sum of G = dL/d(out), (H, W, C)
    out = rasterize_features(F, buffers, H, W)                           # the same image, differentiable in F (torch.autograd)

No background is added (1 - buffers["final_Ts"] is the coverage), geometry is a constant of the call, and nothing is binned or
sorted again.  The forward gives the same bits every call; the backward adds rows with float atomics, so the last bits of dF may
differ from run to run.  A capacity-mode frame is to be used only once rendered_count(buffers) has said that it did not overflow, as
for backward().  Everything is enqueued on the current stream; nothing is read back.
"""
import torch

from . import _args, _frame, _host, _lib

FRAME_KEYS, _masks_of = _frame.FRAME_KEYS, _frame.masks_of      # (they live in _frame.py; still importable under their old names)


def _check_array(t, name, rows, what):
    """A (rows..., C) float32 contiguous device tensor; returns C."""
    lead = tuple(rows)
    if not (_args.is_dev(t, torch.float32) and t.dim() == len(lead) + 1 and tuple(t.shape[:-1]) == lead):
        raise ValueError(f"{name} must be a float32 device tensor of shape {what}")
    c = int(t.shape[-1])
    if not 1 <= c <= _lib.FEATURES_MAX_CHANNELS:
        raise ValueError(f"{name}: the number of channels must lie in [1, {_lib.FEATURES_MAX_CHANNELS}] (got {c})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return c


def render_features(features, buffers, image_height, image_width, out=None, *, use_block_masks=True):
    """(H, W, C) float32: out[y, x, c] = sum over the pixel's contributing list entries of w_k * features[i_k, c], front to back.
    `features`: contiguous float32 (N, C) device tensor, N the frame's, 1 <= C <= 64.  `out`: a caller-owned tensor to write into
    (every element is written).  use_block_masks=False walks without the forward's block masks (the same bits either way)."""
    fr = _frame.Frame.from_buffers(buffers, image_height, image_width, use_block_masks)
    c = _check_array(features, "features", (fr.N,), "(N, C) with N the frame's number of Gaussians")
    out, = fr.outputs(out, [(fr.H, fr.W, c)], (features,))
    if fr.N == 0:
        return out.zero_()
    src = _host.to_dev(features, torch.float32, fr.device)     # itself, or an aligned copy of an offset view
    fr.launch("gsr_features_forward", c, _host.ptr(src), _host.ptr(out), written=(out,))
    return out


def render_features_backward(dL_dout, buffers, image_height, image_width, out=None, *, use_block_masks=True):
    """(N, C) float32: dL_dF[i, c] = sum over pixels of w_i(p) * dL_dout[p, c].  `dL_dout`: contiguous float32 (H, W, C) device
    tensor.  `out`: a caller-owned (N, C) tensor; it is written, not added to, and rows of Gaussians no pixel used are exactly 0."""
    fr = _frame.Frame.from_buffers(buffers, image_height, image_width, use_block_masks)
    c = _check_array(dL_dout, "dL_dout", (fr.H, fr.W), "(H, W, C)")
    out, = fr.outputs(out, [(fr.N, c)], (dL_dout,))
    if fr.N == 0:
        return out
    src = _host.to_dev(dL_dout, torch.float32, fr.device)      # itself, or an aligned copy of an offset view
    fr.launch("gsr_features_backward", c, _host.ptr(src), _host.ptr(out), written=(out,))
    return out


class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, buffers, image_height, image_width):
        ctx.frame = (buffers, image_height, image_width)
        return render_features(features.detach(), buffers, image_height, image_width)

    @staticmethod
    @torch.autograd.function.once_differentiable      # the library call is a constant to autograd: a double backward is refused
    def backward(ctx, dL_dout):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        buffers, H, W = ctx.frame
        return render_features_backward(dL_dout.contiguous(), buffers, H, W), None, None, None


def rasterize_features(features, buffers, image_height, image_width):
    """render_features() as a torch.autograd.Function, differentiable in `features` (the frame is a constant): optimise features
    on a frozen model with any torch optimiser."""
    fr = _frame.Frame.from_buffers(buffers, image_height, image_width, use_block_masks=False)    # (refused here, before autograd sees the call)
    _check_array(features, "features", (fr.N,), "(N, C) with N the frame's number of Gaussians")
    return _Rasterize.apply(features, buffers, image_height, image_width)
