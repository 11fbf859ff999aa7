"""The yardsticks of include/gsr_mesh_eval.h and 3dgs-native_amd/mesh_eval.py, in numpy, written from the header's text.

    nearest_reference(q, r, max_dist2)      a chunked float32 brute force: d2 = (dx * dx + dy * dy) + dz * dz in that order (numpy
                                            contracts nothing), candidates d2 <= max_dist2, the first in (d2, j) order; (inf, -1) without one
    sample_reference(tri, density, seed)    (offsets (T + 1,) int32, points (S, 3) float32, tri_index (S,) int32): the hash, the float32
                                            area, the stochastically rounded count and the samples, every step one rounded operation
    evaluate_reference(pred, gt, ...)       accuracy / completeness / chamfer / precision / recall / fscore in float64 from the float32 d2

Used bit for bit by tests/test_gpu_mesh_eval.py and held to closed forms by tests/test_mesh_eval_reference.py."""
import numpy as np

F = np.float32
MAX_PER_TRIANGLE = 1 << 20          # the header's GSR_SURFACE_SAMPLE_MAX_PER_TRIANGLE


def nearest_reference(queries, refs, max_dist2=np.inf, chunk=None):
    """(dist2 (M,) float32, index (M,) int32)."""
    q = np.ascontiguousarray(queries, F).reshape(-1, 3)
    r = np.ascontiguousarray(refs, F).reshape(-1, 3)
    m, n = len(q), len(r)
    cap = F(max_dist2)
    d2, idx = np.empty(m, F), np.empty(m, np.int32)
    chunk = chunk or max(1, min(m, (1 << 23) // n))            # about 8 M distances at a time
    for a in range(0, m, chunk):
        b = min(m, a + chunk)
        dx = q[a:b, None, 0] - r[None, :, 0]
        dy = q[a:b, None, 1] - r[None, :, 1]
        dz = q[a:b, None, 2] - r[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F
        j = np.argmin(d, axis=1)                               # the first occurrence of the minimum: the lowest index among ties
        best = d[np.arange(b - a), j]
        ok = best <= cap                                       # the nearest reference is a candidate, or nothing is
        d2[a:b] = np.where(ok, best, F(np.inf))
        idx[a:b] = np.where(ok, j, -1)
    return d2, idx


# ---- the sampler ----
def mix(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def unit(seed, t, k):
    """u(seed, t, k) in [0, 1) as float32; t and k are arrays that broadcast."""
    with np.errstate(over="ignore"):
        t, k = np.asarray(t).astype(np.uint32), np.asarray(k).astype(np.uint32)
        h = mix(mix(np.uint32(seed) ^ (t * np.uint32(0x9E3779B9))) ^ (k * np.uint32(0x85EBCA6B)))
    return (h >> np.uint32(8)).astype(F) * F(2.0 ** -24)


def triangle_areas(tri):
    """(area (T,) float32 as the header computes it, a, e1, e2)."""
    tri = np.ascontiguousarray(tri, F).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = F(0.5) * np.sqrt((nx * nx + ny * ny) + nz * nz)
    assert area.dtype == F
    return area, a, e1, e2


def sample_counts(tri, density, seed):
    area, _, _, _ = triangle_areas(tri)
    T = len(area)
    with np.errstate(all="ignore"):
        x = np.minimum(area * F(density), F(MAX_PER_TRIANGLE))
        whole = np.floor(x)
        extra = unit(seed, np.arange(T), np.full(T, 0xFFFFFFFF, np.uint32)) < (x - whole)
    ok = np.isfinite(area)
    return np.where(ok, np.where(ok, whole, 0).astype(np.int64) + extra, 0).astype(np.int64)


def sample_reference(tri, density, seed):
    tri = np.ascontiguousarray(tri, F).reshape(-1, 3, 3)
    counts = sample_counts(tri, density, seed)
    T = len(counts)
    offsets = np.zeros(T + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    assert offsets[-1] < 1 << 31
    S = int(offsets[-1])
    t = np.repeat(np.arange(T), counts)
    j = np.arange(S) - offsets[:-1][t]
    _, a, e1, e2 = triangle_areas(tri)
    r1, r2 = unit(seed, t, 2 * j), unit(seed, t, 2 * j + 1)
    flip = (r1 + r2) > F(1)
    r1, r2 = np.where(flip, F(1) - r1, r1), np.where(flip, F(1) - r2, r2)
    with np.errstate(all="ignore"):
        p = (a[t] + r1[:, None] * e1[t]) + r2[:, None] * e2[t]
    assert p.dtype == F
    return offsets.astype(np.int32), p.reshape(S, 3), t.astype(np.int32)


# ---- the metrics ----
def evaluate_reference(pred, gt, thresholds, max_dist=None, bounds=None):
    """The dict of mesh_eval.evaluate, every sum in float64 over the float32 d2 of nearest_reference."""
    pred, gt = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (pred, gt))
    if bounds is not None:
        lo, hi = (np.asarray(b, np.float64).astype(F) for b in bounds)
        pred, gt = (x[((x >= lo) & (x <= hi)).all(axis=1)] for x in (pred, gt))
    with np.errstate(over="ignore"):
        cap = F(np.inf) if max_dist is None else F(float(max_dist) * float(max_dist))

    def one_way(q, r):
        d2, _ = nearest_reference(q, r, cap)
        found = np.isfinite(d2)
        d = np.sqrt(d2.astype(np.float64))
        with np.errstate(all="ignore"):
            mean = d[found].sum() / found.sum()
        return float(mean), float((len(q) - found.sum()) / len(q)), [float((d <= t).sum() / len(q)) for t in thresholds]

    acc, out_p, prec = one_way(pred, gt)
    comp, out_g, rec = one_way(gt, pred)
    return {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "thresholds": [float(t) for t in thresholds], "precision": prec,
            "recall": rec, "fscore": [2.0 * p * r / (p + r) if p + r > 0.0 else 0.0 for p, r in zip(prec, rec)], "n_pred": len(pred), "n_gt": len(gt),
            "outlier_pred": float(out_p), "outlier_gt": float(out_g)}


# ---- scenes ----
def sphere_mesh(radius, grid, half=1.0):
    """The triangle soup (T, 3, 3) float32 of a sphere about the origin, extracted by the TSDF yardstick from the analytic signed
    distance on a grid^3 volume over [-half, half]^3; also the voxel size h."""
    import tsdf_reference as TR
    h = 2.0 * half / (grid - 1)
    vol = TR.fill_sdf(TR.new_volume((-half, -half, -half), h, (grid, grid, grid), color=False), TR.sphere_sdf((0.0, 0.0, 0.0), radius))
    verts, _, _, _ = TR.extract(vol, 1.0)
    return verts, h


def sphere_bounds(delta, density, h, radius):
    """[delta - b, sqrt(delta^2 + s^2) + b]: what the mean distance between samples of two concentric sphere meshes, radii R and
    R + delta, lies in.  s = 1 / sqrt(density) is twice the mean spacing of the samples; b = 3 h^2 / (8 R) bounds how far the
    extraction's linear interpolation over an edge of at most sqrt(3) h leaves the sphere (a chord's sagitta)."""
    b = 3.0 * h * h / (8.0 * radius)
    s = 1.0 / np.sqrt(density)
    return delta - b, float(np.sqrt(delta * delta + s * s) + b)
