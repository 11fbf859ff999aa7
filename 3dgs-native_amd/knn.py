"""
Exact 3-nearest-neighbour distances of a point cloud (include/gsr_knn.h) over the MI355X library: what a 3DGS run that starts from
SfM points, or from random ones, sizes its Gaussians by.

    mean_dist2 = knn(points)                            # (N,) float32: mean squared distance to the 3 nearest other points
    mean_dist2, indices = knn(points, want_indices=True)    # ... and their indices, (N, 3) int32, -1 where N - 1 < 3
    scales = init_scales(points)                        # (N, 3) raw scales: sqrt(max(mean_dist2, floor)) on all three axes

The result is defined exactly (float32, the order of operations and the tie-break by index are in the header): the Morton order and
the block boxes inside the library only prune.  Everything is enqueued on the current stream; nothing is read back.
"""
import torch

from . import _args, _host, _lib


def _check_points(points):
    if not isinstance(points, torch.Tensor):
        raise ValueError(f"points must be a torch tensor (got {type(points).__name__})")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32 (got {points.dtype})")
    if not points.is_cuda:
        raise ValueError("points must live on the GPU (device tensor)")
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"points must have shape (N, 3) with N >= 1 (got {tuple(points.shape)})")
    if points.shape[0] > _lib.KNN_MAX_POINTS:
        raise ValueError(f"points: at most {_lib.KNN_MAX_POINTS} points (got {points.shape[0]})")
    if not points.is_contiguous():
        raise ValueError("points must be contiguous")
    return int(points.shape[0])


def knn(points, want_indices=False, out=None):
    """mean_dist2 (N,) float32 of the contiguous float32 (N, 3) device tensor `points`; with want_indices also the neighbours'
    indices (N, 3) int32 in (distance, index) order, as a pair.  `out`: caller-owned tensors to write into -- the (N,) float32
    tensor, or with want_indices the pair ((N,) float32, (N, 3) int32)."""
    N = _check_points(points)
    mean, idx = None, None
    if out is not None:
        if want_indices:
            if not (isinstance(out, (tuple, list)) and len(out) == 2):
                raise ValueError("out must be the pair (mean_dist2, indices) when want_indices is set")
            mean, idx = out
            _args.check_out(idx, (N, 3), "out[1] (indices)", torch.int32)
        else:
            mean = out
        _args.check_out(mean, (N,), "out (mean_dist2)" if not want_indices else "out[0] (mean_dist2)")
    L = _lib.lib()
    dev = points.device
    points = _host.to_dev(points, torch.float32, dev)      # itself, or an aligned copy of an offset view such as cloud[1:]
    if mean is None:
        mean = torch.empty((N,), dtype=torch.float32, device=dev)
    if want_indices and idx is None:
        idx = torch.empty((N, 3), dtype=torch.int32, device=dev)
    stream = _host.raw_stream(dev)
    with _host.on_device(dev):
        ws = _host.workspace("knn", L.gsr_knn_workspace_bytes(N), dev, stream)
        _lib.check(L.gsr_knn(N, _host.ptr(points), _host.ptr(mean), _host.ptr(idx), _host.ptr(ws), ws.numel(), stream))
    _host.written_in_place(mean, idx)
    return (mean, idx) if want_indices else mean


def init_scales(points, floor=1e-7):
    """(N, 3) raw scales for Gaussians at `points`: sqrt(max(mean_dist2, floor)) on all three axes -- the original's
    `sqrt(clamp_min(distCUDA2(points), 1e-7))`, without its log: this project's scales are raw (quirk Q5)."""
    floor = _args.positive(floor, "floor", allow_inf=True)
    return torch.sqrt(torch.clamp_min(knn(points), floor)).unsqueeze(1).repeat(1, 3)
