"""
Mesh evaluation (include/gsr_mesh_eval.h) over the MI355X library: points sampled on a triangle mesh by area, the exact nearest
neighbour of every point of one set in another, and the three numbers surface-reconstruction methods report from them -- accuracy,
completeness (together the Chamfer distance) and the F-score at a distance threshold.

    d2 = nearest(queries, refs, max_dist=inf)                      # (M,) float32 squared distances; +inf where nothing is within max_dist
    d2, idx = nearest(queries, refs, want_indices=True)            # ... and the references' indices, (M,) int32, -1 where none
    pts, tri = sample_mesh(triangles, density=100.0)               # (S, 3) float32 points on the (T, 3, 3) soup, (S,) int32 triangle of each
    pts, tri = sample_mesh(triangles, samples=1_000_000)           # density = samples / total area: about that many
    m = evaluate(pred_points, gt_points, thresholds=(0.01, 0.02), max_dist=None, bounds=None)

Both results are defined exactly (float32, the order of operations, the tie-break by index and the random numbers are in the header):
the Morton order and the block boxes inside the library only prune.  Everything is enqueued on the current stream.  nearest reads
nothing back; sample_mesh reads two numbers back (the total area, to bound the sample count before the call, and the count): sampling
is an offline step.  evaluate reads its sums back.
"""
import math

import numpy as np
import torch

from . import _args, _host, _lib


def _check_points(points, name, device_only=True):
    if not isinstance(points, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor (got {type(points).__name__})")
    if points.dtype != torch.float32:
        raise ValueError(f"{name} must be float32 (got {points.dtype})")
    if device_only and not points.is_cuda:
        raise ValueError(f"{name} must live on the GPU (device tensor)")
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"{name} must have shape (N, 3) with N >= 1 (got {tuple(points.shape)})")
    if points.shape[0] > _lib.NEAREST_MAX_POINTS:
        raise ValueError(f"{name}: at most {_lib.NEAREST_MAX_POINTS} points (got {points.shape[0]})")
    if not points.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return int(points.shape[0])


def cap2(max_dist, max_dist2=None):
    """The float32 max_dist2 the library receives: `max_dist2` itself, or max_dist * max_dist formed in float64 and rounded once."""
    if max_dist2 is not None:
        if not (max_dist is None or (isinstance(max_dist, float) and math.isinf(max_dist) and max_dist > 0)):
            raise ValueError("give max_dist or max_dist2, not both")
        v = _args._number(max_dist2, "max_dist2")
    else:
        v = _args._number(max_dist, "max_dist")
        v = v * v if v >= 0.0 else v
    if not v >= 0.0:
        raise ValueError(f"{'max_dist2' if max_dist2 is not None else 'max_dist'} must be >= 0 or inf, not {max_dist2 if max_dist2 is not None else max_dist}")
    with np.errstate(over="ignore"):
        return float(np.float32(v))


def nearest(queries, refs, max_dist=float("inf"), want_indices=False, out=None, max_dist2=None):
    """dist2 (M,) float32: for every row of the contiguous float32 (M, 3) device tensor `queries` the squared distance to its nearest
    row of `refs` (N, 3) among those within max_dist (squared distance <= max_dist2; give `max_dist2` instead of `max_dist` to
    state the float32 cap exactly), +inf where there is none.  With want_indices also that row's index (M,) int32, -1 where none, as
    a pair; ties go to the lower index.  `out`: caller-owned tensors to write into -- the (M,) float32 tensor, or with want_indices
    the pair ((M,) float32, (M,) int32)."""
    M = _check_points(queries, "queries")
    N = _check_points(refs, "refs")
    _args.check_one_device(queries, refs)
    cap = cap2(max_dist, max_dist2)
    d2, idx = None, None
    if out is not None:
        if want_indices:
            if not (isinstance(out, (tuple, list)) and len(out) == 2):
                raise ValueError("out must be the pair (dist2, indices) when want_indices is set")
            d2, idx = out
            _args.check_out(idx, (M,), "out[1] (indices)", torch.int32)
        else:
            d2 = out
        _args.check_out(d2, (M,), "out (dist2)" if not want_indices else "out[0] (dist2)")
    L = _lib.lib()
    dev = queries.device
    queries = _host.to_dev(queries, torch.float32, dev)        # itself, or an aligned copy of an offset view such as cloud[1:]
    refs = _host.to_dev(refs, torch.float32, dev)
    if d2 is None:
        d2 = torch.empty((M,), dtype=torch.float32, device=dev)
    if want_indices and idx is None:
        idx = torch.empty((M,), dtype=torch.int32, device=dev)
    stream = _host.raw_stream(dev)
    with _host.on_device(dev):
        ws = _host.workspace("nearest", L.gsr_nearest_workspace_bytes(M, N), dev, stream)
        _lib.check(L.gsr_nearest(M, _host.ptr(queries), N, _host.ptr(refs), cap, _host.ptr(d2), _host.ptr(idx), _host.ptr(ws), ws.numel(), stream))
    _host.written_in_place(d2, idx)
    return (d2, idx) if want_indices else d2


def _check_triangles(triangles, who):
    if not isinstance(triangles, (torch.Tensor, np.ndarray)):
        raise ValueError(f"{who}: triangles must be a torch tensor or a numpy array, not {type(triangles).__name__}")
    shape = tuple(triangles.shape)
    if len(shape) != 3 or shape[1:] != (3, 3) or shape[0] < 1:
        raise ValueError(f"{who}: triangles must have shape (T, 3, 3) with T >= 1 (got {shape})")
    if not _args.is_f32(triangles):
        raise ValueError(f"{who}: triangles must be float32, not {triangles.dtype}")
    if shape[0] > _lib.SURFACE_SAMPLE_MAX_TRIANGLES:
        raise ValueError(f"{who}: at most {_lib.SURFACE_SAMPLE_MAX_TRIANGLES} triangles (got {shape[0]})")
    return shape[0]


def soup(verts, faces):
    """An indexed mesh (verts (V, 3), faces (T, 3) integers) as the (T, 3, 3) float32 numpy triangle soup sample_mesh takes."""
    v = np.ascontiguousarray(np.asarray(verts, np.float32)).reshape(-1, 3)
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu" or (len(f) and (f.min() < 0 or f.max() >= len(v))):
        raise ValueError("soup: faces must be (T, 3) integer indices into verts")
    return np.ascontiguousarray(v[f.astype(np.int64)])


def total_area(triangles):
    """The float64 sum of the finite triangle areas of a (T, 3, 3) tensor, as a 0-dim tensor on its device (no host read)."""
    t = triangles.to(torch.float64)
    a = 0.5 * torch.linalg.norm(torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), dim=1)
    return torch.where(torch.isfinite(a), a, torch.zeros_like(a)).sum()


def sample_mesh(triangles, density=None, samples=None, seed=0, device=None):
    """(points (S, 3) float32, tri_index (S,) int32) device tensors: random points on the triangle soup `triangles` (T, 3, 3) float32,
    `density` of them per unit area in expectation -- floor(area * density) per triangle plus one more with the probability of the
    remainder -- or about `samples` in all (density = samples / total area).  Exactly one of the two.  Triangle order, then sample
    order; a triangle with a non-finite vertex gets none.  The same arguments give the same bits."""
    who = "sample_mesh"
    T = _check_triangles(triangles, who)
    if (density is None) == (samples is None):
        raise ValueError(f"{who}: give exactly one of density and samples")
    if density is not None:
        density = _args.positive(density, f"{who}: density")
    else:
        if isinstance(samples, bool) or int(samples) != samples or not 1 <= samples <= _lib.SURFACE_SAMPLE_MAX_SAMPLES:
            raise ValueError(f"{who}: samples must be an integer in 1 .. {_lib.SURFACE_SAMPLE_MAX_SAMPLES}, not {samples!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 32:
        raise ValueError(f"{who}: seed must be an integer in 0 .. 2^32 - 1, not {seed!r}")
    L = _lib.lib()
    dev = torch.device(device) if device is not None else _host.device_of(triangles)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    tri = _host.to_dev(triangles, torch.float32, dev, (T, 3, 3))
    area = float(total_area(tri).item())                       # the first host read: it bounds the count before anything is sized
    if density is None:
        if not area > 0.0:
            raise ValueError(f"{who}: the mesh has no area to spread {samples} samples over")
        density = float(samples) / area
    with np.errstate(over="ignore"):
        d32 = float(np.float32(density))
    if not (d32 > 0.0 and math.isfinite(d32)):
        raise ValueError(f"{who}: density must be positive and finite in float32, not {density}")
    if area * d32 * (1.0 + 1e-6) + T >= float(1 << 31):
        raise ValueError(f"{who}: about {area * d32:.3g} samples: the count must stay below 2^31")
    offsets = torch.empty((T + 1,), dtype=torch.int32, device=dev)
    stream = _host.raw_stream(dev)
    with _host.on_device(dev):
        ws = _host.workspace("surface_sample", L.gsr_surface_sample_workspace_bytes(T), dev, stream)
        _lib.check(L.gsr_surface_sample_count(T, _host.ptr(tri), d32, int(seed), _host.ptr(offsets), _host.ptr(ws), ws.numel(), stream))
        S = int(offsets[T].item())                             # the second host read: the count
        if not 0 <= S <= _lib.SURFACE_SAMPLE_MAX_SAMPLES:
            raise ValueError(f"{who}: {S} samples: at most {_lib.SURFACE_SAMPLE_MAX_SAMPLES} in one call (lower the density)")
        points = torch.empty((S, 3), dtype=torch.float32, device=dev)
        index = torch.empty((S,), dtype=torch.int32, device=dev)
        if S > 0:
            _lib.check(L.gsr_surface_sample_emit(T, _host.ptr(tri), _host.ptr(offsets), int(seed), S, _host.ptr(points), _host.ptr(index), stream))
    return points, index


def _cloud(x, name):
    if isinstance(x, np.ndarray):
        if x.dtype != np.float32:
            raise ValueError(f"{name} must be float32 (got {x.dtype})")
        x = torch.from_numpy(np.array(x, order="C"))            # a copy: the caller's array may be read-only
    _check_points(x, name, device_only=False)
    return x


def check_evaluate(thresholds, max_dist, bounds):
    """(thresholds as a list of floats, max_dist or None, (lo, hi) float32 arrays or None), judged before the GPU is touched."""
    try:
        taus = [float(t) for t in thresholds]
    except (TypeError, ValueError):
        taus = []
    if not taus or not all(t > 0.0 and math.isfinite(t) for t in taus):
        raise ValueError(f"evaluate: thresholds must be one or more positive finite distances, not {thresholds!r}")
    if max_dist is not None:
        max_dist = _args.positive(max_dist, "evaluate: max_dist", allow_inf=True)
    if bounds is not None:
        try:
            lo, hi = (np.asarray(b, np.float64).reshape(-1) for b in bounds)
            ok = lo.shape == hi.shape == (3,) and bool((lo <= hi).all())
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"evaluate: bounds must be (lo, hi), two points with lo <= hi, not {bounds!r}")
        bounds = (lo.astype(np.float32), hi.astype(np.float32))
    return taus, max_dist, bounds


def _one_way(d2, taus):
    """(sum of the distances of the points with a neighbour, how many have one, how many lie within each tau) as one float64 device
    tensor: counts are exact in float64, and the divisions are the host's."""
    found = torch.isfinite(d2)
    d = torch.sqrt(d2.to(torch.float64))
    total = torch.where(found, d, torch.zeros_like(d)).sum()
    return torch.stack([total, found.sum().to(torch.float64)] + [(d <= t).sum().to(torch.float64) for t in taus])


def evaluate(pred_points, gt_points, thresholds=(0.01, 0.02, 0.05), max_dist=None, bounds=None):
    """The geometric error of `pred_points` (P, 3) against `gt_points` (G, 3), float32 torch tensors or numpy arrays, as a dict:
    accuracy (the mean distance pred -> gt), completeness (gt -> pred), chamfer (their mean), and per threshold tau, in the order
    given, precision (the share of pred points within tau of gt), recall (the share of gt points within tau of pred) and
    fscore = 2 P R / (P + R) (0 when both are 0); thresholds, n_pred, n_gt, outlier_pred, outlier_gt.
    With `max_dist`, points without a neighbour within it are left out of the two means, counted in the outlier shares, and misses
    for precision and recall (the DTU convention).  `bounds` = (lo, hi) crops both sets to that box first.  Distances are the square
    roots, taken in float64, of gsr_nearest's float32 squared distances; the sums are float64."""
    taus, max_dist, bounds = check_evaluate(thresholds, max_dist, bounds)
    clouds = [(_cloud(x, f"evaluate: {name}"), name) for x, name in ((pred_points, "pred_points"), (gt_points, "gt_points"))]
    dev = _host.device_of(pred_points, gt_points)
    sets = []
    for x, name in clouds:
        x = x.to(dev)
        if bounds is not None:
            lo, hi = (torch.from_numpy(b).to(dev) for b in bounds)
            x = x[((x >= lo) & (x <= hi)).all(dim=1)]
            if x.shape[0] < 1:
                raise ValueError(f"evaluate: no point of {name} lies inside bounds")
        sets.append(x.contiguous())
    pred, gt = sets
    cap = float("inf") if max_dist is None else max_dist
    a = _one_way(nearest(pred, gt, max_dist=cap), taus)
    c = _one_way(nearest(gt, pred, max_dist=cap), taus)
    a, c = a.tolist(), c.tolist()                              # the host reads
    n_pred, n_gt = int(pred.shape[0]), int(gt.shape[0])
    acc = a[0] / a[1] if a[1] > 0 else float("nan")
    comp = c[0] / c[1] if c[1] > 0 else float("nan")
    prec, rec = [h / n_pred for h in a[2:]], [h / n_gt for h in c[2:]]
    return {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "thresholds": taus, "precision": prec, "recall": rec,
            "fscore": [2.0 * p * r / (p + r) if p + r > 0.0 else 0.0 for p, r in zip(prec, rec)], "n_pred": n_pred, "n_gt": n_gt,
            "outlier_pred": (n_pred - a[1]) / n_pred, "outlier_gt": (n_gt - c[1]) / n_gt}
