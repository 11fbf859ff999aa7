"""The mesh-evaluation yardsticks (tests/mesh_eval_reference.py) against cases known in closed form: what the GPU test compares bit
for bit must itself be the definition of include/gsr_mesh_eval.h.  Also load_mesh_ply, which needs no GPU."""
import functools

import numpy as np
import pytest

from conftest import sub
from mesh_eval_reference import (evaluate_reference, nearest_reference, sample_counts, sample_reference, sphere_bounds, sphere_mesh, triangle_areas,
                                 unit)
from test_knn_reference import lattice

SEED = 0                    # fixed once, before the first run: the statistical bounds below are p = 0.001 statements about THIS stream
UNIT = np.array([[[0.0, 0.0, 0.25], [1.0, 0.0, 0.25], [0.0, 1.0, 0.25]]], np.float32)      # the unit right triangle: area 1/2


def centres(n=8, pitch=0.25):
    """The (n - 1)^3 cell centres of lattice(n, pitch), x fastest; exact in float32."""
    g = (np.arange(n - 1, dtype=np.float32) + np.float32(0.5)) * np.float32(pitch)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


CORNER_D2 = np.float32(3 * 0.125 * 0.125)      # a cell centre to each of its eight corners, exact


def test_eight_equidistant_references_the_lowest_index_wins():
    r, q = lattice(), centres()
    d2, idx = nearest_reference(q, r)
    assert d2.dtype == np.float32 and idx.dtype == np.int32
    assert (d2 == CORNER_D2).all()
    cx, cy, cz = np.meshgrid(np.arange(7), np.arange(7), np.arange(7), indexing="ij")   # z, y, x order of `centres`
    assert idx.tolist() == (cz.ravel() + 8 * cy.ravel() + 64 * cx.ravel()).tolist()      # the cell's own corner: the lowest of the eight
    small = nearest_reference(q, r, chunk=5)                   # the chunking changes nothing
    assert small[0].tobytes() == d2.tobytes() and small[1].tobytes() == idx.tobytes()


def test_queries_on_references_and_duplicate_references():
    r = lattice()
    d2, idx = nearest_reference(r, r)
    assert (d2 == 0).all() and idx.tolist() == list(range(512))
    dup = np.concatenate([r[100:101], r, r[100:101]])          # reference 100 now also stands at index 0 and at the end
    d2, idx = nearest_reference(r[100:101], dup)
    assert d2.tolist() == [0.0] and idx.tolist() == [0]
    d2, idx = nearest_reference(np.full((4, 3), 0.37, np.float32), np.full((300, 3), 0.37, np.float32))
    assert (d2 == 0).all() and (idx == 0).all()


def test_the_cap_keeps_a_tie_at_the_cap_and_drops_it_one_ulp_below():
    r, q = lattice(), centres()
    d2, idx = nearest_reference(q, r, CORNER_D2)
    assert (d2 == CORNER_D2).all() and idx[0] == 0 and (idx >= 0).all()
    d2, idx = nearest_reference(q, r, np.nextafter(CORNER_D2, np.float32(0)))
    assert np.isposinf(d2).all() and (idx == -1).all()
    d2, idx = nearest_reference(np.concatenate([q[:3], r[:2]]), r, 0.0)                   # cap 0: only a query ON a reference finds it
    assert d2.tolist() == [np.inf] * 3 + [0.0, 0.0] and idx.tolist() == [-1, -1, -1, 0, 1]


def test_float32_arithmetic_in_the_stated_order():
    # dx^2 + dy^2 = 2^24 exactly, + dz^2 = 1 is lost in float32; a float64 sum, or dz first, would keep it
    q = np.array([[4096.0, 0.0, 1.0]], np.float32)
    d2, _ = nearest_reference(q, np.zeros((1, 3), np.float32))
    assert d2.tolist() == [float(1 << 24)]


# ---- the sampler ----
def random_triangles(n, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (n, 1, 3)) + rng.normal(0, 0.05, (n, 3, 3))).astype(np.float32)


def test_the_hash_is_the_headers():
    assert unit(0, 0, 0).dtype == np.float32
    u = unit(SEED, np.arange(1000), np.arange(1000)[::-1])
    assert (u >= 0).all() and (u < 1).all() and len(np.unique(u)) > 990
    # mix by hand for one input: seed 1, t 2, k 3
    def m(x):
        x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
        return x
    h = m(m(1 ^ ((2 * 0x9E3779B9) & 0xFFFFFFFF)) ^ ((3 * 0x85EBCA6B) & 0xFFFFFFFF))
    assert float(unit(1, 2, 3)) == (h >> 8) / float(1 << 24)


def test_every_sample_lies_inside_its_triangle_in_triangle_order():
    tri = random_triangles(5000)
    offsets, p, t = sample_reference(tri, 2000.0, SEED)
    assert offsets.dtype == np.int32 and p.dtype == np.float32 and t.dtype == np.int32
    assert offsets[0] == 0 and offsets[-1] == len(p) == len(t) and (np.diff(t) >= 0).all()
    assert (np.bincount(t, minlength=5000) == np.diff(offsets)).all()
    a, e1, e2 = (x.astype(np.float64) for x in triangle_areas(tri)[1:])
    d = p.astype(np.float64) - a[t]
    # barycentric coordinates by least squares in float64; float32 rounding of p moves them by about 1e-7 / edge length
    G = np.stack([np.stack([(e1 * e1).sum(1), (e1 * e2).sum(1)], 1), np.stack([(e1 * e2).sum(1), (e2 * e2).sum(1)], 1)], 1)[t]
    uv = np.linalg.solve(G, np.stack([(d * e1[t]).sum(1), (d * e2[t]).sum(1)], 1)[..., None])[..., 0]
    assert uv.min() > -1e-4 and uv.sum(1).max() < 1 + 1e-4
    off_plane = np.linalg.norm(d - uv[:, :1] * e1[t] - uv[:, 1:] * e2[t], axis=1)
    assert off_plane.max() < 1e-5


def test_stochastic_rounding_keeps_the_expected_total():
    tri = random_triangles(5000)
    for density in (200.0, 2000.0):
        area = triangle_areas(tri)[0]
        want = (area * np.float32(density)).astype(np.float64).sum()
        got = sample_counts(tri, density, SEED).sum()
        print(f"density {density}: total {got}, expected {want:.1f}, {(got - want) / np.sqrt(5000 / 4):+.2f} sigma")
        assert abs(got - want) < 4 * np.sqrt(5000 / 4)         # a sum of 5 000 Bernoulli remainders: variance at most T / 4


def test_one_triangle_is_covered_uniformly():
    _, p, _ = sample_reference(UNIT, 20000.0, SEED)            # area 1/2: exactly 10 000 samples, no remainder
    n = len(p)
    assert n == 10000 and (p[:, 2] == np.float32(0.25)).all()
    sigma = np.sqrt(1.0 / 18.0) / np.sqrt(n)                   # a coordinate of a uniform point of the unit right triangle has variance 1/18
    c = p[:, :2].astype(np.float64).mean(0)
    print("centroid off by", ((c - 1 / 3) / sigma).round(2), "sigma")
    assert (np.abs(c - 1.0 / 3.0) < 4 * sigma).all()
    u, v = p[:, 0], p[:, 1]
    which = np.where(u > 0.5, 0, np.where(v > 0.5, 1, np.where(u + v < 0.5, 2, 3)))      # the four midpoint sub-triangles, equal areas
    obs = np.bincount(which, minlength=4)
    chi2 = float(((obs - n / 4) ** 2 / (n / 4)).sum())
    print("sub-triangle counts", obs.tolist(), "chi-square", round(chi2, 2))
    assert chi2 < 16.27                                        # 3 degrees of freedom, p = 0.001


def test_degenerate_nan_and_huge_triangles():
    tri = np.concatenate([UNIT, UNIT * 0, UNIT, UNIT * np.float32(3000)])
    tri[2, 1, 0] = np.nan
    counts = sample_counts(tri, 1.0, SEED)
    assert counts[1] == 0 and counts[2] == 0 and counts[3] == 1 << 20                     # zero area, a NaN vertex, the clamp (4.5e6 wanted)
    assert counts[0] in (0, 1)


# ---- the metrics ----
R_SPHERE, DELTA, GRID, HALF, DENSITY = 0.5, 0.05, 25, 0.75, 2000.0


@functools.lru_cache(maxsize=None)
def sphere_clouds():
    """Samples of the two extracted sphere meshes, radii R and R + delta; computed once, shared, never written."""
    inner, h = sphere_mesh(R_SPHERE, GRID, HALF)
    outer, _ = sphere_mesh(R_SPHERE + DELTA, GRID, HALF)
    a, b = sample_reference(inner, DENSITY, SEED)[1], sample_reference(outer, DENSITY, SEED + 1)[1]
    for x in (a, b):
        x.setflags(write=False)
    return a, b, h


def test_concentric_spheres_are_delta_apart():
    a, b, h = sphere_clouds()
    lo, hi = sphere_bounds(DELTA, DENSITY, h, R_SPHERE)
    m = evaluate_reference(a, b, thresholds=(10 * DELTA, DELTA / 10))
    print(f"accuracy {m['accuracy']:.5f} completeness {m['completeness']:.5f} in [{lo:.5f}, {hi:.5f}]; n = {m['n_pred']}, {m['n_gt']}")
    assert lo <= m["accuracy"] <= hi and lo <= m["completeness"] <= hi
    assert m["chamfer"] == 0.5 * (m["accuracy"] + m["completeness"])
    assert m["fscore"] == [1.0, 0.0] and m["precision"] == [1.0, 0.0] and m["recall"] == [1.0, 0.0]
    assert m["outlier_pred"] == m["outlier_gt"] == 0.0
    assert abs(m["n_pred"] - 4 * np.pi * R_SPHERE ** 2 * DENSITY) < 0.02 * m["n_pred"]


def test_max_dist_and_bounds():
    a, b, h = sphere_clouds()
    # a cap below delta - b: nothing has a neighbour, everything is an outlier and a miss
    m = evaluate_reference(a, b, thresholds=(1.0,), max_dist=0.5 * DELTA)
    assert m["outlier_pred"] == m["outlier_gt"] == 1.0 and m["precision"] == m["recall"] == m["fscore"] == [0.0]
    assert np.isnan(m["accuracy"]) and np.isnan(m["completeness"])
    # the upper half only, and a far point in pred that the cap sets aside
    pred = np.concatenate([a, [[0.0, 0.0, 5.0]]]).astype(np.float32)
    m = evaluate_reference(pred, b, thresholds=(2 * DELTA,), max_dist=0.5)
    lo, hi = sphere_bounds(DELTA, DENSITY, h, R_SPHERE)
    assert lo <= m["accuracy"] <= hi and m["outlier_pred"] == 1.0 / len(pred) and m["precision"] == [(len(pred) - 1) / len(pred)]
    c = evaluate_reference(pred, b, thresholds=(2 * DELTA,), bounds=((-1, -1, 0.2), (1, 1, 1)))
    assert c["n_pred"] == int((a[:, 2] >= np.float32(0.2)).sum()) and c["n_gt"] == int((b[:, 2] >= np.float32(0.2)).sum())
    assert lo <= c["accuracy"] <= hi and c["outlier_pred"] == 0.0
    same = evaluate_reference(a, a, thresholds=(1e-9,))
    assert same["accuracy"] == same["completeness"] == same["chamfer"] == 0.0 and same["fscore"] == [1.0]


def test_mesh_ply_round_trips(tmp_path):
    pc = sub("point_cloud")
    rng = np.random.default_rng(7)
    v = rng.normal(0, 1, (40, 3)).astype(np.float32)
    f = rng.integers(0, 40, (75, 3)).astype(np.int32)
    c = (rng.integers(0, 256, (40, 3)) / 255.0).astype(np.float32)
    p = str(tmp_path / "m.ply")
    pc.save_mesh_ply(p, v, f)
    V, Fc, C = pc.load_mesh_ply(p)
    assert V.dtype == np.float32 and Fc.dtype == np.int32 and V.tobytes() == v.tobytes() and Fc.tobytes() == f.tobytes() and C is None
    pc.save_mesh_ply(p, v, f, c)
    V, Fc, C = pc.load_mesh_ply(p)
    assert V.tobytes() == v.tobytes() and Fc.tobytes() == f.tobytes() and C.dtype == np.float32 and np.abs(C - c).max() <= 1 / 255 + 1e-7
    pc.save_mesh_ply(p, v, np.zeros((0, 3), np.int32))
    assert pc.load_mesh_ply(p)[1].shape == (0, 3)
    soup = sub("mesh_eval").soup(v, f)
    assert soup.shape == (75, 3, 3) and soup.dtype == np.float32 and (soup[3, 1] == v[f[3, 1]]).all()
    # refused: truncated, ASCII, a quad, another list type, an index outside, no faces element, no PLY
    pc.save_mesh_ply(p, v, f)
    size = len(open(p, "rb").read())
    with open(p, "r+b") as fh:
        fh.truncate(size - 1)
    with pytest.raises(ValueError, match="truncated"):
        pc.load_mesh_ply(p)
    head = "ply\nformat {} 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\nproperty list {} vertex_indices\nend_header\n"
    body = np.zeros((4, 3), "<f4").tobytes()

    def write(fmt="binary_little_endian", lst="uchar int", face=b"\x03" + np.array([0, 1, 2], "<i4").tobytes(), header=None):
        with open(p, "wb") as fh:
            fh.write((header or head.format(fmt, lst)).encode("ascii") + body + face)
    write()
    assert pc.load_mesh_ply(p)[1].tolist() == [[0, 1, 2]]
    write(fmt="ascii")
    with pytest.raises(ValueError, match="binary_little_endian"):
        pc.load_mesh_ply(p)
    write(face=b"\x04" + np.array([0, 1, 2], "<i4").tobytes())
    with pytest.raises(ValueError, match="triangle"):
        pc.load_mesh_ply(p)
    write(lst="uchar short")
    with pytest.raises(ValueError, match="list uchar int"):
        pc.load_mesh_ply(p)
    write(face=b"\x03" + np.array([0, 1, 4], "<i4").tobytes())
    with pytest.raises(ValueError, match="outside"):
        pc.load_mesh_ply(p)
    write(header="ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    with pytest.raises(ValueError, match="face element"):
        pc.load_mesh_ply(p)
    with open(p, "wb") as fh:
        fh.write(b"solid\n")
    with pytest.raises(ValueError, match="not a PLY"):
        pc.load_mesh_ply(p)
