"""The mesh-evaluation stage on the MI355X against its numpy yardsticks (tests/mesh_eval_reference.py).  gsr_nearest and the sampler
are defined exactly by include/gsr_mesh_eval.h, so they are compared BIT FOR BIT, no tolerance: on the shapes on which a pruned
search can go wrong (wave and block edges on either side, one Morton cell, zero-extent axes, outliers that stretch the grid, massive
ties, queries outside the references' box, the cap at, below and above a tie), then the properties the definition implies
(determinism, independence from the workspace's contents and the stream).  evaluate is held to the float64 yardstick at 1e-10
relative (n eps64 for 10^6 terms: the order of a float64 sum differs between torch and numpy), the extraction of an analytic sphere
to the bounds derived in mesh_eval_reference.sphere_bounds, and the torus demonstration to finite, positive numbers."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
from mesh_eval_reference import evaluate_reference, nearest_reference, sample_reference, sphere_bounds
from test_gpu_knn import mixture
from test_knn_reference import lattice
from test_mesh_eval_reference import CORNER_D2, DELTA, DENSITY, GRID, HALF, R_SPHERE, SEED, UNIT, centres, random_triangles, sphere_clouds

pytestmark = pytest.mark.gpu
B = sub("_lib").NEAREST_BLOCK_POINTS
INF = np.float32(np.inf)
SIZES = (1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1)


def uniform(n, seed, lo=-1.3, hi=1.3):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


def flat(n, seed, axis):
    p = uniform(n, seed)
    p[:, axis] = np.float32(0.25)
    return p


def with_outlier(n, seed):
    return np.concatenate([uniform(n, seed, 0, 1), [[1e4, 1e4, 1e4]]]).astype(np.float32)


def two_clusters(seed):
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0, 1e-3, (200, 3)), rng.uniform(0, 1e-3, (200, 3)) + 1e3
    return np.concatenate([a, b]).astype(np.float32)[rng.permutation(400)]


def _equal_to_refs():
    r = uniform(700, 30)
    return r[np.random.default_rng(31).permutation(700)[:300]], r, INF


# name -> (queries, references, max_dist2)
CASES = {
    "one_reference_2049_queries": lambda: (uniform(8 * B + 1, 10), uniform(1, 11), INF),
    "2049_references_one_query": lambda: (uniform(1, 12), uniform(8 * B + 1, 13), INF),
    "identical_300_references": lambda: (uniform(500, 14), np.full((300, 3), 0.37, np.float32), INF),       # two blocks of duplicates: index 0 everywhere
    "references_in_one_morton_cell": lambda: (uniform(600, 15), (np.float32(0.5) + uniform(600, 16, 0, 1e-5)).astype(np.float32), INF),
    "queries_in_one_morton_cell": lambda: ((np.float32(0.5) + uniform(600, 17, 0, 1e-5)).astype(np.float32), uniform(600, 18), INF),
    "flat_references": lambda: (uniform(700, 19), flat(700, 20, 2), INF),
    "flat_queries": lambda: (flat(700, 21, 0), uniform(700, 22), INF),
    "both_flat_on_one_axis": lambda: (flat(300, 23, 1), flat(700, 24, 1), INF),
    "outlier_among_references": lambda: (uniform(1000, 25, 0, 1), with_outlier(2000, 26), INF),
    "outlier_among_queries": lambda: (with_outlier(1000, 27), uniform(2000, 28, 0, 1), INF),
    "two_tight_clusters": lambda: (np.random.default_rng(29).uniform(0, 1e-3, (300, 3)).astype(np.float32), two_clusters(2), INF),
    "queries_above_the_references_box": lambda: (uniform(700, 32, 2, 3), uniform(1500, 33, 0, 1), INF),      # the seed is the last block
    "queries_below_the_references_box": lambda: (uniform(700, 34, -3, -2), uniform(1500, 35, 0, 1), INF),    # ... the first
    "queries_equal_to_references": _equal_to_refs,
    "tie_lattice": lambda: (centres(), lattice(), INF),
    "tie_lattice_cap_0": lambda: (np.concatenate([centres(), lattice()[::7]]), lattice(), np.float32(0)),
    "tie_lattice_cap_below_every_distance": lambda: (centres(), lattice(), np.float32(1e-3)),
    "tie_lattice_cap_at_the_tie": lambda: (centres(), lattice(), CORNER_D2),
    "tie_lattice_cap_one_ulp_below": lambda: (centres(), lattice(), np.nextafter(CORNER_D2, np.float32(0))),
    "mixture_cap_splits_the_queries": lambda: (mixture(8 * B + 1, seed=40), mixture(8 * B + 1, seed=41), np.float32(1e-3)),
    f"mixture_{8 * B + 1}": lambda: (mixture(8 * B + 1, seed=42), mixture(8 * B + 1, seed=43), INF),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(queries, references, cap, yardstick dist2, yardstick index): computed once, shared, never written."""
    q, r, cap = CASES[name]()
    d2, idx = nearest_reference(q, r, cap)
    for a in (q, r, d2, idx):
        a.setflags(write=False)
    return q, r, cap, d2, idx


def run(q, r, cap=INF, want_indices=True):
    me = sub("mesh_eval")
    out = me.nearest(torch.tensor(q).cuda(), torch.tensor(r).cuda(), max_dist2=float(cap), want_indices=want_indices)
    torch.cuda.synchronize()
    if want_indices:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy(), None


def differing(got, ref):
    bad = np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0]
    return f"{len(bad)} of {len(got)} differ, first {bad[:5].tolist()}: got {got[bad[:3]].tolist()} want {ref[bad[:3]].tolist()}"


def check(q, r, cap, d2, idx):
    got_d2, got_idx = run(q, r, cap)
    assert got_d2.dtype == np.float32 and got_idx.dtype == np.int32 and got_d2.shape == got_idx.shape == (len(q),)
    assert got_d2.tobytes() == d2.tobytes(), differing(got_d2, d2)
    assert got_idx.tobytes() == idx.tobytes(), differing(got_idx, idx)
    only_d2, _ = run(q, r, cap, want_indices=False)             # index = NULL: the same distances
    assert only_d2.tobytes() == d2.tobytes(), differing(only_d2, d2)


@pytest.mark.parametrize("name", list(CASES))
def test_nearest_matches_the_yardstick_bit_for_bit(name):
    check(*case(name))


@pytest.mark.parametrize("m", SIZES)
def test_nearest_at_wave_and_block_edges_on_either_side(m):
    q = uniform(m, 100 + m)
    for n in SIZES:
        r = uniform(n, 200 + n)
        check(q, r, INF, *nearest_reference(q, r))


def test_closed_forms_on_the_device():
    q, r, _, _, _ = case("tie_lattice")
    d2, idx = run(q, r)
    assert (d2 == CORNER_D2).all() and idx[:3].tolist() == [0, 1, 2] and idx[7] == 8
    d2, idx = run(q, r, np.nextafter(CORNER_D2, np.float32(0)))
    assert np.isposinf(d2).all() and (idx == -1).all()
    d2, idx = run(*case("identical_300_references")[:2])
    assert (idx == 0).all()
    d2, idx = run(np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]], np.float32), np.array([[1.0, 2.0, 2.0]], np.float32))
    assert d2.tolist() == [9.0, 0.0] and idx.tolist() == [0, 0]


def test_many_blocks_values_only():
    """16 385 x 16 385 points of the mixture, 65 blocks on either side, through the NULL path; the yardstick takes a few seconds."""
    q, r = mixture(16385, seed=6), mixture(16385, seed=7)
    d2, _ = nearest_reference(q, r)
    got, _ = run(q, r, want_indices=False)
    assert got.tobytes() == d2.tobytes(), differing(got, d2)


def test_same_bits_every_call_whatever_the_workspace_held_and_on_a_side_stream():
    _host, _lib, me = sub("_host"), sub("_lib"), sub("mesh_eval")
    q, r, _, d2, idx = case(f"mixture_{8 * B + 1}")
    qt, rt = torch.tensor(q).cuda(), torch.tensor(r).cuda()
    dev = qt.device
    first = me.nearest(qt, rt, want_indices=True)
    again = me.nearest(qt, rt, want_indices=True)
    ws = _host.workspace("nearest", _lib.lib().gsr_nearest_workspace_bytes(len(q), len(r)), dev)
    ws.fill_(0xFF)
    dirty = me.nearest(qt, rt, want_indices=True)
    assert _host.workspace("nearest", 1, dev) is ws            # (the call above ran in the workspace that was filled)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aside = me.nearest(qt, rt, want_indices=True)
    torch.cuda.synchronize()
    for name, (d, i) in (("first", first), ("again", again), ("0xFF workspace", dirty), ("side stream", aside)):
        assert d.cpu().numpy().tobytes() == d2.tobytes(), name
        assert i.cpu().numpy().tobytes() == idx.tobytes(), name
    out = (torch.empty(len(q), device=dev), torch.empty(len(q), dtype=torch.int32, device=dev))
    assert me.nearest(qt, rt, want_indices=True, out=out)[0] is out[0]
    torch.cuda.synchronize()
    assert out[0].cpu().numpy().tobytes() == d2.tobytes() and out[1].cpu().numpy().tobytes() == idx.tobytes()
    by_distance = me.nearest(qt, rt, max_dist=0.25)            # max_dist is squared in float64 and rounded once
    torch.cuda.synchronize()
    assert by_distance.cpu().numpy().tobytes() == nearest_reference(q, r, np.float32(0.0625))[0].tobytes()


# ---- the sampler ----
def special_triangles():
    tri = np.concatenate([random_triangles(3, seed=8), UNIT * 0, UNIT, UNIT * np.float32(3000), random_triangles(2, seed=9)])
    tri[4, 1, 0] = np.nan
    return tri          # 3: zero area; 4: a NaN vertex; 5: 4.5e6 samples wanted at density 1, clamped to 2^20


SAMPLER_CASES = {**{f"random_{t}": (functools.partial(random_triangles, t, seed=50 + t), 2000.0) for t in (1, 63, 64, 65, 1025)},
                 "degenerate_nan_and_the_clamp": (special_triangles, 1.0),
                 "most_counts_are_zero": (functools.partial(random_triangles, 1025, seed=60), 20.0)}


def sample(tri, **kw):
    pts, idx = sub("mesh_eval").sample_mesh(torch.tensor(tri).cuda(), **kw)
    torch.cuda.synchronize()
    return pts.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("name", list(SAMPLER_CASES))
def test_sampler_matches_the_yardstick_bit_for_bit(name):
    make, density = SAMPLER_CASES[name]
    tri = make()
    offsets, p, t = sample_reference(tri, density, SEED)
    pts, idx = sample(tri, density=density, seed=SEED)
    assert pts.dtype == np.float32 and idx.dtype == np.int32 and pts.shape == (len(p), 3) and idx.shape == (len(p),)
    assert idx.tobytes() == t.tobytes()
    assert pts.tobytes() == p.tobytes(), f"{int((pts.view(np.uint32) != p.view(np.uint32)).any(axis=1).sum())} of {len(p)} points differ"
    if name == "degenerate_nan_and_the_clamp":
        counts = np.diff(offsets)
        assert counts[3] == 0 and counts[4] == 0 and counts[5] == 1 << 20
    if name == "most_counts_are_zero":
        assert (np.diff(offsets) == 0).mean() > 0.5 and len(p) > 0


def test_offsets_capacity_and_seeds():
    _host, _lib = sub("_host"), sub("_lib")
    L = _lib.lib()
    tri = random_triangles(1025, seed=70)
    offsets, p, t = sample_reference(tri, 2000.0, SEED)
    S, T = len(p), len(tri)
    dev = torch.device("cuda", torch.cuda.current_device())
    tri_d = torch.tensor(tri).cuda()
    off_d = torch.empty(T + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.gsr_surface_sample_workspace_bytes(T)), dtype=torch.uint8, device=dev).fill_(0xFF)
    stream = _host.raw_stream(dev)
    _lib.check(L.gsr_surface_sample_count(T, tri_d.data_ptr(), 2000.0, SEED, off_d.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    assert off_d.cpu().numpy().tobytes() == offsets.tobytes()
    # a capacity below S: nothing at or beyond it is written, in either output; tri_index may be NULL
    cap = S - 300
    pts = torch.full((S, 3), -7.0, device=dev)
    idx = torch.full((S,), -7, dtype=torch.int32, device=dev)
    _lib.check(L.gsr_surface_sample_emit(T, tri_d.data_ptr(), off_d.data_ptr(), SEED, cap, pts.data_ptr(), idx.data_ptr(), stream))
    torch.cuda.synchronize()
    assert pts[:cap].cpu().numpy().tobytes() == p[:cap].tobytes() and idx[:cap].cpu().numpy().tobytes() == t[:cap].tobytes()
    assert bool((pts[cap:] == -7.0).all()) and bool((idx[cap:] == -7).all())
    pts.fill_(-7.0)
    _lib.check(L.gsr_surface_sample_emit(T, tri_d.data_ptr(), off_d.data_ptr(), SEED, S, pts.data_ptr(), None, stream))
    torch.cuda.synchronize()
    assert pts.cpu().numpy().tobytes() == p.tobytes()
    # the same seed: the same bits; another seed: other points; `samples`: about that many
    again, _ = sample(tri, density=2000.0, seed=SEED)
    other, _ = sample(tri, density=2000.0, seed=SEED + 1)
    assert again.tobytes() == p.tobytes()
    n = min(len(other), S)
    assert abs(len(other) - S) < 4 * np.sqrt(T / 2) and (other[:n] != p[:n]).any(axis=1).mean() > 0.9
    about, _ = sample(tri, samples=5000, seed=SEED)
    assert abs(len(about) - 5000) < 4 * np.sqrt(T / 4) + 1


# ---- evaluate ----
def close(got, want):
    for k, w in want.items():
        g = got[k]
        if isinstance(w, list):
            assert len(g) == len(w) and all(abs(a - b) <= 1e-10 * abs(b) for a, b in zip(g, w)), (k, g, w)
        elif isinstance(w, int):
            assert g == w, (k, g, w)
        elif np.isnan(w):
            assert np.isnan(g), (k, g, w)
        else:
            assert abs(g - w) <= 1e-10 * abs(w), (k, g, w)


def test_evaluate_matches_the_float64_yardstick():
    me = sub("mesh_eval")
    a, b, _ = sphere_clouds()
    pred = np.concatenate([a, [[0.0, 0.0, 5.0]]]).astype(np.float32)
    taus = (0.5 * DELTA, DELTA, 2 * DELTA)
    for kw in ({}, {"max_dist": 1.02 * DELTA}, {"bounds": ((-1, -1, 0.2), (1, 1, 1))}, {"max_dist": 0.5, "bounds": ((-0.3, -1, -1), (1, 1, 6))}):
        want = evaluate_reference(pred, b, taus, **kw)
        close(me.evaluate(pred, torch.tensor(b).cuda(), thresholds=taus, **kw), want)
        assert 0 < want["precision"][1] < 1 and want["n_pred"] > 1000        # (the thresholds and the crop cut through the data)
    capped = evaluate_reference(pred, b, taus, max_dist=1.02 * DELTA)
    assert 0 < capped["outlier_pred"] < 1 and 0 < capped["outlier_gt"] < 1
    same = me.evaluate(a, a, thresholds=(1e-9, 1.0))
    assert same["accuracy"] == same["completeness"] == same["chamfer"] == 0.0 and same["fscore"] == [1.0, 1.0]
    assert same["outlier_pred"] == same["outlier_gt"] == 0.0 and same["n_pred"] == same["n_gt"] == len(a)


def test_an_extracted_sphere_is_delta_from_the_larger_sphere():
    """End to end on the device: the analytic sphere SDF in a TSDFVolume, extracted, welded, sampled and evaluated against samples of
    the sphere of radius R + delta (the yardstick's), held to the bounds the CPU test holds the yardstick to."""
    import tsdf_reference as TR
    me, tsdf = sub("mesh_eval"), sub("tsdf")
    h = 2.0 * HALF / (GRID - 1)
    vol = tsdf.TSDFVolume((-HALF, -HALF, -HALF), h, (GRID, GRID, GRID), color=False)
    ref = TR.fill_sdf(TR.new_volume((-HALF, -HALF, -HALF), h, (GRID, GRID, GRID), color=False), TR.sphere_sdf((0.0, 0.0, 0.0), R_SPHERE))
    vol.tsdf.copy_(torch.from_numpy(ref["tsdf"]))
    vol.weight.fill_(1.0)
    vertices, _, keys = vol.extract_mesh(1.0)
    verts, faces, _ = tsdf.weld(vertices, keys)
    pts, _ = me.sample_mesh(me.soup(verts, faces), density=DENSITY, seed=SEED)
    _, outer, _ = sphere_clouds()
    m = me.evaluate(pts, outer, thresholds=(10 * DELTA, DELTA / 10))
    lo, hi = sphere_bounds(DELTA, DENSITY, h, R_SPHERE)
    print(f"accuracy {m['accuracy']:.5f} completeness {m['completeness']:.5f} in [{lo:.5f}, {hi:.5f}]; n = {m['n_pred']}, {m['n_gt']}")
    assert lo <= m["accuracy"] <= hi and lo <= m["completeness"] <= hi
    assert m["fscore"] == [1.0, 0.0] and abs(m["n_pred"] - 4 * np.pi * R_SPHERE ** 2 * DENSITY) < 0.02 * m["n_pred"]


def test_the_torus_demonstration_ends_with_finite_positive_metrics(tmp_path):
    out = str(tmp_path / "torus.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "eval_mesh.py"), "--demo", "torus", "--resolution", "64", "--views", "8",
                        "--json", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    m = json.load(open(out))
    print({k: m[k] for k in ("accuracy_voxels", "completeness_voxels", "chamfer", "fscore", "n_pred", "n_gt", "triangles")})
    for k in ("accuracy", "completeness", "chamfer", "accuracy_voxels", "completeness_voxels", "voxel_size"):
        assert np.isfinite(m[k]) and m[k] > 0, k
    assert m["demo"] == "torus" and m["resolution"] == 64 and m["views"] == 8 and m["triangles"] > 0 and m["n_pred"] > 0 and m["n_gt"] > 0
    assert len(m["thresholds"]) == len(m["precision"]) == len(m["recall"]) == len(m["fscore"]) and all(0 <= f <= 1 for f in m["fscore"])
