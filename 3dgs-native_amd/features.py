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
import ctypes as C
import numbers

import torch

from . import _args, _host, _lib
from .config import TILE_M, TILE_N

FRAME_KEYS = ("points_xy_image", "conic_opacity", "point_list", "ranges", "n_contrib")


def _check_frame(buffers, H, W):
    """The frame's arrays, checked against W and H; returns (N, D, xy, conic_opacity, point_list, ranges, n_contrib)."""
    if isinstance(H, bool) or isinstance(W, bool) or not isinstance(H, numbers.Integral) or not isinstance(W, numbers.Integral):
        raise ValueError("image_height and image_width must be integers")
    H, W = int(H), int(W)
    if not (1 <= H <= _lib.FEATURES_MAX_SIDE and 1 <= W <= _lib.FEATURES_MAX_SIDE):
        raise ValueError(f"image_height and image_width must lie in [1, {_lib.FEATURES_MAX_SIDE}] (got {H} x {W})")
    if not isinstance(buffers, dict) or any(k not in buffers for k in FRAME_KEYS):
        raise ValueError(f"buffers must be the dict render_gaussians returned (with {', '.join(FRAME_KEYS)})")
    xy, co, pl, rg, nc = (buffers[k] for k in FRAME_KEYS)
    for name, t, width in (("points_xy_image", xy, 2), ("conic_opacity", co, 4)):
        # the strided column views of the blend records, or packed arrays: rows of `width` consecutive floats, any row stride
        if not (_args.is_dev(t, torch.float32) and t.dim() == 2 and t.shape[1] == width and (t.shape[0] == 0 or (t.stride(1) == 1 and t.stride(0) >= width))):
            raise ValueError(f"buffers['{name}'] must be a float32 device tensor of shape (N, {width}) with unit stride along its rows")
    N = int(xy.shape[0])
    if int(co.shape[0]) != N:
        raise ValueError("buffers['points_xy_image'] and buffers['conic_opacity'] disagree on the number of Gaussians")
    if not (_args.is_dev(pl, torch.int32) and pl.dim() == 1 and pl.is_contiguous()):
        raise ValueError("buffers['point_list'] must be a contiguous int32 device tensor of shape (D,)")
    tiles = ((W + TILE_M - 1) // TILE_M) * ((H + TILE_N - 1) // TILE_N)
    if not (_args.is_dev(rg, torch.int32) and tuple(rg.shape) == (tiles, 2) and rg.is_contiguous()):
        raise ValueError(f"buffers['ranges'] must be a contiguous int32 device tensor of shape ({tiles}, 2) for a {W} x {H} image")
    if not (_args.is_dev(nc, torch.int32) and tuple(nc.shape) == (H, W) and nc.is_contiguous()):
        raise ValueError(f"buffers['n_contrib'] must be a contiguous int32 device tensor of shape ({H}, {W})")
    D = int(pl.shape[0])
    if D > _lib.MAX_RENDERED:
        raise ValueError("buffers['point_list'] holds more than 2^30 entries")
    return N, D, xy, co, pl, rg, nc


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


def _masks_of(buffers, D, dev):
    """The forward blend's block masks, when `buffers` is that forward's own dict with every array they describe unwritten."""
    tag = getattr(buffers["point_list"], "_gsr_block_masks", None)
    if tag is None:
        return None
    m, stamps, _ = tag
    given = {"ranges": buffers["ranges"], "n_contrib": buffers["n_contrib"], "final_Ts": buffers.get("final_Ts"),
             "means2D": buffers["points_xy_image"], "conic_opacity": buffers["conic_opacity"]}
    if (all(_host.unwritten(stamps[k], given.get(k)) for k in stamps) and isinstance(m, torch.Tensor) and m.dtype == torch.uint8
            and m.device == dev and m.numel() == D and m.is_contiguous()):
        return m
    return None


def _call(entry, src, dst, frame_args, C_, use_masks):
    N, D, xy, co, pl, rg, nc = frame_args
    dev = src.device
    _args.check_one_device(src, xy, co, pl, rg, nc, dst)
    src = _host.to_dev(src, torch.float32, dev)     # itself, or an aligned copy of an offset view
    L = _lib.lib()
    masks = use_masks if isinstance(use_masks, torch.Tensor) else None
    H, W = int(nc.shape[0]), int(nc.shape[1])
    frame = _lib.GsrFeaturesFrame(W, H, N, D, xy.data_ptr(), int(xy.stride(0)), co.data_ptr(), int(co.stride(0)), _host.ptr(pl), _host.ptr(rg),
                                  _host.ptr(nc), _host.ptr(masks))
    with _host.on_device(dev):
        _lib.check(getattr(L, entry)(C.byref(frame), C_, _host.ptr(src), _host.ptr(dst), _host.raw_stream(dev)))
    _host.written_in_place(dst)
    return dst


def render_features(features, buffers, image_height, image_width, out=None, *, use_block_masks=True):
    """(H, W, C) float32: out[y, x, c] = sum over the pixel's contributing list entries of w_k * features[i_k, c], front to back.
    `features`: contiguous float32 (N, C) device tensor, N the frame's, 1 <= C <= 64.  `out`: a caller-owned tensor to write into
    (every element is written).  use_block_masks=False walks without the forward's block masks (the same bits either way)."""
    fr = _check_frame(buffers, image_height, image_width)
    c = _check_array(features, "features", (fr[0],), "(N, C) with N the frame's number of Gaussians")
    shape = (int(image_height), int(image_width), c)
    if out is not None:
        _args.check_out(out, shape, "out")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=features.device)
    if fr[0] == 0:
        return out.zero_()
    return _call("gsr_features_forward", features, out, fr, c, _masks_of(buffers, fr[1], features.device) if use_block_masks else None)


def render_features_backward(dL_dout, buffers, image_height, image_width, out=None, *, use_block_masks=True):
    """(N, C) float32: dL_dF[i, c] = sum over pixels of w_i(p) * dL_dout[p, c].  `dL_dout`: contiguous float32 (H, W, C) device
    tensor.  `out`: a caller-owned (N, C) tensor; it is written, not added to, and rows of Gaussians no pixel used are exactly 0."""
    fr = _check_frame(buffers, image_height, image_width)
    c = _check_array(dL_dout, "dL_dout", (int(image_height), int(image_width)), "(H, W, C)")
    shape = (fr[0], c)
    if out is not None:
        _args.check_out(out, shape, "out")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dL_dout.device)
    if fr[0] == 0:
        return out
    return _call("gsr_features_backward", dL_dout, out, fr, c, _masks_of(buffers, fr[1], dL_dout.device) if use_block_masks else None)


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
    fr = _check_frame(buffers, image_height, image_width)       # (refused here, before autograd sees the call)
    _check_array(features, "features", (fr[0],), "(N, C) with N the frame's number of Gaussians")
    return _Rasterize.apply(features, buffers, image_height, image_width)
