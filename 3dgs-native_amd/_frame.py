"""The host counterpart of csrc/frame_walk.h: the finished frame every stage that replays its tile lists reads (features,
distortion, normal_render, median_depth, plane_depth and the stages of backward()), as one checked record.  It is made from the
dict a forward returned (Frame.from_buffers) or from the records backward() blended with (Frame.from_records), and turned into
the library's struct in one place (Frame.struct)."""
import ctypes as C
import numbers

import torch

from . import _args, _host, _lib
from .config import TILE_M, TILE_N

FRAME_KEYS = ("points_xy_image", "conic_opacity", "point_list", "ranges", "n_contrib")


def masks_of(buffers, D, dev):
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


def inv_depth_of(buffers, N, dev):
    """(N,) float32 view or tensor of 1 / view depth: column 9 of the forward's blend records while the frame's arrays are theirs
    and unwritten, else 1 / buffers['depths'] (0 where the depth is not positive, as the records have it)."""
    xy = buffers["points_xy_image"]
    tag = getattr(xy, "_gsr_records", None)
    if tag is not None:
        rec, stamps = tag
        given = {"means2D": xy, "conic_opacity": buffers["conic_opacity"], "rgb": buffers.get("colors")}
        if all(_host.unwritten(stamps[k], given.get(k)) for k in stamps) and rec.device == dev and tuple(rec.shape) == (N, 16):
            return rec[:, 9]
    d = buffers.get("depths")
    if not (_args.is_dev(d, torch.float32) and d.dim() == 1 and d.shape[0] == N):
        raise ValueError("buffers['depths'] must be a float32 device tensor of shape (N,) when the frame does not carry the forward's records")
    return torch.where(d > 0, 1.0 / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(d))


class Frame:
    """N Gaussians, D list entries, a W x H image; the five checked arrays; the forward's block masks or None; the (N,) column of
    1 / depth or None (a stage that does not read it)."""
    __slots__ = ("N", "D", "W", "H", "xy", "conic_opacity", "point_list", "ranges", "n_contrib", "masks", "inv_depth", "device")

    def __init__(self, N, D, W, H, xy, conic_opacity, point_list, ranges, n_contrib, masks, inv_depth, device):
        self.N, self.D, self.W, self.H = N, D, W, H
        self.xy, self.conic_opacity, self.point_list, self.ranges, self.n_contrib = xy, conic_opacity, point_list, ranges, n_contrib
        self.masks, self.inv_depth, self.device = masks, inv_depth, device

    @classmethod
    def from_buffers(cls, buffers, H, W, use_block_masks=True, inv_depth=False):
        """The frame of a forward's `buffers`, its arrays checked against W and H.  `inv_depth`: the stage reads 1 / depth
        (inv_depth_of).  A frame with no Gaussians is never walked: it looks for neither the masks nor 1 / depth."""
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
        dev, walked = xy.device, N > 0
        return cls(N, D, W, H, xy, co, pl, rg, nc, masks_of(buffers, D, dev) if use_block_masks and walked else None,
                   inv_depth_of(buffers, N, dev) if inv_depth and walked else None, dev)

    @classmethod
    def from_records(cls, rec, point_list, ranges, n_contrib, masks):
        """The frame backward() blended with: the (N, 16) records (the forward's own, or the re-packed ones at the head of the
        workspace) give xy, conic_opacity and 1 / depth as column views; the lists, ranges, counts and masks are that call's."""
        H, W = n_contrib.shape
        return cls(int(rec.shape[0]), int(point_list.numel()), int(W), int(H), rec[:, 0:2], rec[:, 2:6], point_list, ranges, n_contrib, masks,
                   rec[:, 9], rec.device)

    def struct(self, inv_depth=True):
        """GsrDistortionFrame when the frame carries 1 / depth (and the stage reads it: `inv_depth`), GsrFeaturesFrame otherwise."""
        xy, co, m = self.xy, self.conic_opacity, self.inv_depth
        head = (self.W, self.H, self.N, self.D, xy.data_ptr(), int(xy.stride(0)), co.data_ptr(), int(co.stride(0)), _host.ptr(self.point_list),
                _host.ptr(self.ranges), _host.ptr(self.n_contrib), _host.ptr(self.masks))
        if m is None or not inv_depth:
            return _lib.GsrFeaturesFrame(*head)
        return _lib.GsrDistortionFrame(*head, m.data_ptr(), int(m.stride(0)))

    def outputs(self, out, shapes, inputs=(), pair=None, dtypes=(torch.float32, torch.float32)):
        """A stage's outputs, one per shape: the caller's `out`, checked -- one tensor, or with `pair` (the pair's name in
        the refusal) a pair -- or fresh tensors; all on one device with the frame's arrays and the stage's `inputs`."""
        if out is None:
            _args.check_one_device(*inputs, self.xy, self.conic_opacity, self.point_list, self.ranges, self.n_contrib)
            if pair is None:
                return (torch.empty(shapes[0], dtype=dtypes[0], device=self.device),)
            return torch.empty(shapes[0], dtype=dtypes[0], device=self.device), torch.empty(shapes[1], dtype=dtypes[1], device=self.device)
        if pair is None:
            out = (out,)
        elif not (isinstance(out, (tuple, list)) and len(out) == 2):
            raise ValueError(f"out must be a {pair} pair")
        for k, (t, shape, dtype) in enumerate(zip(out, shapes, dtypes)):
            _args.check_out(t, shape, "out" if pair is None else f"out[{k}]", dtype=dtype)
        _args.check_one_device(*inputs, self.xy, self.conic_opacity, self.point_list, self.ranges, self.n_contrib, *out)
        return tuple(out)

    def launch(self, entry, *args, written=()):
        """On the frame's device and torch's current stream: the library's `entry`(the frame by reference, *args, stream), its status
        checked; `written` are the tensors it wrote through raw pointers."""
        L = _lib.lib()
        frame = self.struct()
        with _host.on_device(self.device):
            _lib.check(getattr(L, entry)(C.byref(frame), *args, _host.raw_stream(self.device)))
        _host.written_in_place(*written)
